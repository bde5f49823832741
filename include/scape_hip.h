/*
 * scape_hip.h - C ABI of libscape_hip.so, the MI355X (gfx950) implementation of
 * SCAPE's `infer_pa` hot path.
 *
 * Conventions
 *   - plain pointers and sizes only; the CALLER owns every host buffer, the library
 *     owns device memory behind an opaque context (one context per GPU);
 *   - every entry point returns 0 on success, non-zero on error;
 *     scape_hip_last_error() returns the message of the calling thread's last error;
 *   - calls on one context are not re-entrant (one host thread per context): a call that arrives while
 *     another is in flight on the same context fails with an error; use one context per thread;
 *   - all floating point is IEEE f64; SCAPE_SENT is the reference's finite "-inf"
 *     (np.finfo('f').min, reference src/scape/taichi_core.py:8, apa_core.py:428).
 *
 * Reference interface replaced (paths relative to the reference checkout):
 *   operator level : src/scape/apa_core.py:23 imports four host functions from
 *                    src/scape/taichi_core.py (:183, :200, :210, :237); the four
 *                    scape_hip_loglik_* / scape_hip_get_loglik_marginal_tensor entry
 *                    points below take the same arrays and return the same arrays.
 *   batched level  : the per-UTR body of ApaModel.run (apa_core.py:930-981) -
 *                    Phase A (:954-957), Phase B (:959), em_algo (:714-779) and
 *                    get_label (:873-881) - for many UTRs at once.
 */
#ifndef SCAPE_HIP_H
#define SCAPE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCAPE_HIP_ABI_VERSION 4
#define SCAPE_SENT (-3.4028234663852886e38)
#define SCAPE_MAX_BETA 160   /* max len(predef_beta_arr): beta_step >= 0.44 at the default max_beta = 70 (ABI 3: 64) */
#define SCAPE_MAX_S 64       /* max len(s_dis_arr)       */
#define SCAPE_MAX_K 63       /* max number of pA components per model (K+1 <= 64; ABI 3: 31) */
#define SCAPE_MAX_JOBS_PER_UTR 1024  /* max non-fixed jobs on one UTR in one scape_hip_batch_em call */

typedef struct scape_hip_ctx scape_hip_ctx;

/* model constants shared by every UTR of a batch (ApaModel.__init__, apa_core.py:333-437) */
typedef struct scape_hip_params {
    double mu_f;            /* apa_core.py:399 */
    double sigma_f;         /* apa_core.py:400 */
    double max_unif_ws;     /* apa_core.py:414 */
    int32_t n_beta;         /* len(predef_beta_arr), apa_core.py:942 */
    int32_t n_s;            /* len(s_dis_arr), apa_core.py:394 */
    int32_t nround;         /* ApaModel.nround = 50, apa_core.py:422 */
    int32_t reserved;
    double betas[SCAPE_MAX_BETA];
    double s_dis[SCAPE_MAX_S];
    double pmf_s[SCAPE_MAX_S];
} scape_hip_params;

int scape_hip_abi_version(void);
const char *scape_hip_last_error(void);
int scape_hip_device_count(int *count);
int scape_hip_create(int device, scape_hip_ctx **out);
int scape_hip_destroy(scape_hip_ctx *ctx);
int scape_hip_device_name(scape_hip_ctx *ctx, char *buf, int buflen);

/* ---- operator level: the taichi_core seam ------------------------------------------- */
/* taichi_core.py:183-197 loglik_xlr_t_pa(x_arr, l_arr, pa_arr, theta, sigma_f) -> out[n] */
int scape_hip_loglik_xlr_t_pa(scape_hip_ctx *ctx, const double *x, const double *l,
                              const double *pa, int32_t n, double theta, double sigma_f,
                              double *out);
/* taichi_core.py:200-207 loglik_xlr_t_r_known(x, l, r, s_dis, pmf_s, theta, mu_f, sigma_f) */
int scape_hip_loglik_xlr_t_r_known(scape_hip_ctx *ctx, const double *x, const double *l,
                                   const double *r, int32_t n, const double *s_dis,
                                   const double *pmf_s, int32_t n_s, double theta, double mu_f,
                                   double sigma_f, double *out);
/* taichi_core.py:210-215 loglik_xlr_t_r_unknown(x, l, r, s_dis, pmf_s, theta, mu_f, sigma_f);
   r is ignored by the reference kernel too and may be NULL */
int scape_hip_loglik_xlr_t_r_unknown(scape_hip_ctx *ctx, const double *x, const double *l,
                                     const double *r, int32_t n, const double *s_dis,
                                     const double *pmf_s, int32_t n_s, double theta, double mu_f,
                                     double sigma_f, double *out);
/* taichi_core.py:237-246 get_loglik_marginal_tensor(all_theta, predef_beta_arr, loglik_xlr_t_arr)
   loglik_xlr_t_arr is [n_frag, n_theta] row-major, out is [n_theta, n_beta, n_frag] */
int scape_hip_get_loglik_marginal_tensor(scape_hip_ctx *ctx, const double *all_theta,
                                         int32_t n_theta, const double *betas, int32_t n_beta,
                                         const double *loglik_xlr_t_arr, int32_t n_frag,
                                         double *out);

/* ---- batched level -------------------------------------------------------------------- */
/*
 * Upload a batch of binned UTRs (output of bin_data, apa_core.py:285-327).  Ragged arrays:
 * UTR u owns bins [bin_off[u], bin_off[u+1]) of x/l/r/pa/cnt and grid points
 * [theta_off[u], theta_off[u+1]) of all_theta (ascending; apa_core.py:940).  r / pa are NaN
 * where unknown (apa_core.py:439-452).  utr_L = ApaModel.L (apa_core.py:387), min_theta
 * (:407), unif_ll = lik_f0(log=True) (:576-584).  Allocates the Phase-A matrix and the
 * marginal tensor on the device.  Replaces any previously loaded batch.
 */
int scape_hip_batch_load(scape_hip_ctx *ctx, const scape_hip_params *params, int32_t n_utr,
                         const int64_t *bin_off, const double *x, const double *l,
                         const double *r, const double *pa, const double *cnt,
                         const int64_t *theta_off, const double *all_theta,
                         const double *utr_L, const double *min_theta, const double *unif_ll);
/* device bytes the loaded batch needs / the device offers (for sizing waves on the host) */
int scape_hip_batch_bytes(scape_hip_ctx *ctx, int64_t *bytes_batch, int64_t *bytes_free,
                          int64_t *bytes_total);
/* Phase A (apa_core.py:954-957) then Phase B (apa_core.py:959) for every UTR of the batch.  The kernels are queued,
   not awaited: the next call on the context runs behind them, and a device-side consistency failure of the build is
   reported by that call (batch_em / batch_labels / batch_fetch_*). */
int scape_hip_batch_build(scape_hip_ctx *ctx);
/* which form of Phase B the last batch_build of the loaded batch queued (diagnostics / tests; the results do not
   depend on it); an error where no build has run on the loaded batch:
   0 = one kernel (the form of get_loglik_marginal_tensor; non-uniform theta grids, > 16 beta values),
   1 = window tables + per-alpha matrix path, 2 = window tables + log-bin columns + sliding windows (uniform theta grids) */
int scape_hip_batch_phase_b_form(scape_hip_ctx *ctx, int32_t *form);
/*
 * n_jobs em_algo calls (apa_core.py:714-779).  Job j works on UTR job_utr[j] with job_K[j]
 * components from the init (alpha_idx, beta_idx = indices into that UTR's all_theta / betas,
 * ws) and the update order k_arr (gen_k_arr, apa_core.py:653-677); job_fixed[j] != 0 selects
 * mstep_fixed (apa_core.py:552-557).  Tables are padded to kmax / kmax+1 / nround per job.
 * Outputs (same padding): sorted alpha_idx / beta_idx / ws, bic, lb_arr and its length.
 * Limits (checked, an error is returned): kmax <= SCAPE_MAX_K; at most SCAPE_MAX_JOBS_PER_UTR jobs with
 * job_fixed == 0 on any one UTR per call (the reference's own sweep is (n_max_apa - n_min_apa + 1) * 10
 * jobs per UTR, apa_core.py:846-871, :965).
 */
int scape_hip_batch_em(scape_hip_ctx *ctx, int32_t n_jobs, int32_t kmax, const int32_t *job_utr,
                       const int32_t *job_K, const int32_t *job_fixed, const int32_t *alpha_idx,
                       const int32_t *beta_idx, const double *ws, const int8_t *k_arr,
                       int32_t *alpha_idx_out, int32_t *beta_idx_out, double *ws_out,
                       double *bic_out, int32_t *n_lb_out, double *lb_out);
/*
 * lb_out of scape_hip_batch_em may be NULL (ABI version 3): the lb_arr rows (nround doubles per job, 20 MB for the
 * 51,200 jobs of a 512-UTR sweep) then stay on the device, and the caller fetches the rows of the few jobs it keeps -
 * the BIC winners that become Parameters.lb_arr (apa_core.py:760-766, :972) - with this call.  job_idx are indices
 * into the job tables of the LAST scape_hip_batch_em call on this handle; lb_out is [n_sel][nround], rows valid up
 * to that job's n_lb.
 */
int scape_hip_batch_em_fetch_lb(scape_hip_ctx *ctx, int32_t n_sel, const int32_t *job_idx, double *lb_out);
/*
 * get_label (apa_core.py:873-881) for n_sel models: per-bin arg-max of the responsibilities.
 * labels_out is indexed like the batch's bins (bin_off of sel_utr[i]); only the bins of the
 * selected UTRs are written.  The output holds one label per bin, so one call labels at most
 * one model per UTR: a call that names a UTR twice is refused ("labels: a UTR is named twice").
 */
int scape_hip_batch_labels(scape_hip_ctx *ctx, int32_t n_sel, int32_t kmax, const int32_t *sel_utr,
                           const int32_t *sel_K, const int32_t *alpha_idx, const int32_t *beta_idx,
                           const double *ws, int32_t *labels_out);
/* parity-test access to intermediates: A[n_frag, n_theta] and M[n_theta, n_beta, n_frag] of one UTR */
int scape_hip_batch_fetch_loglik(scape_hip_ctx *ctx, int32_t utr, double *A_out);
int scape_hip_batch_fetch_tensor(scape_hip_ctx *ctx, int32_t utr, double *M_out);
int scape_hip_batch_free(scape_hip_ctx *ctx);

/*
 * Kernel timing measured with HIP events on the stream the kernels are launched on.
 * which: 0 = Phase A, 1 = Phase B, 2 = EM (one whole scape_hip_batch_em call), 3 = labels,
 * 4 = the per-round E-step kernel, 5 = the per-round M-step kernel (4 and 5 are recorded only when the
 * environment variable SCAPE_HIP_ROUND_TIMING is set).  Returns the sum of the durations and the number
 * of launches since the last scape_hip_timing_reset().
 */
int scape_hip_timing_reset(scape_hip_ctx *ctx);
int scape_hip_timing_get(scape_hip_ctx *ctx, int32_t which, double *ms_total, int32_t *n_launches);
/* EM work counters of the last scape_hip_batch_em call (for the algorithmic-bytes formula):
   sum over jobs of rounds, and of rounds x window rows x n_beta x n_frag (tensor elements read
   by the grid arg-max M-step, apa_core.py:507-523), and of rounds x n_frag x (K+1) */
int scape_hip_em_counters(scape_hip_ctx *ctx, int64_t *rounds, int64_t *slab_elems,
                          int64_t *z_elems);

/* HBM-side byte tally of the M-step kernel over the last scape_hip_batch_em call, counted by the kernel
   itself: tensor-tile bytes it streamed (each live 64-row tile x the bins it needs, once per round), the
   v-vector bytes as requested by every workgroup (mostly L2 hits) and counted once per (job, round), and
   the number of M-step launches.  Replaces nothing in the reference (measurement only). */
int scape_hip_em_traffic(scape_hip_ctx *ctx, int64_t *mstep_tensor_bytes, int64_t *mstep_v_bytes_requested,
                         int64_t *mstep_v_bytes_unique, int64_t *mstep_launches);

/* ---- reporting stages after merge_pa (report.inc; the three Matrix Market renderers: report_mtx.inc) -------------
 * ex_pa_cnt_mat (reference utils.py:438-553) and cal_exp_pa_len (utils.py:319-427, apa_core.py:1038-1063).  A batch is
 * n_rec records; record r owns reads [read_off[r], read_off[r+1]) of label / cb_id and has K[r] pA sites.  Barcode ids
 * map to columns (or cluster codes) through id2x[cb_id - id_min] for 0 <= cb_id - id_min < id_span, -1 = unknown.
 * bad_read_out[0] is the first read whose id has no column / code (for the matrix: among reads with label < K),
 * bad_read_out[1] the first read with a negative label; -1 if none.  Counts are 32-bit: a record may hold at most
 * INT32_MAX reads.
 */
/* (record, label < K, column) counts, kept on the device for rendering; row_tot_out[sum K] = reads per (record, label)
   (rows of record r start at the sum of K over the records before it); complete_out[r] = 1 when every column with a read
   in record r has reads in every row of r that has reads (the reference's pivot then prints integers) */
int scape_hip_report_counts(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *read_off, const int32_t *K,
                            const int64_t *label, const int64_t *cb_id, int64_t id_min, int64_t id_span,
                            const int32_t *id2col, int32_t n_cols, int64_t *row_tot_out, int8_t *complete_out,
                            int64_t *bad_read_out);
/* Render n_rows CSV rows of the last counts call into slot 0 or 1: row i is the quoted prefix pre[pre_off[i],
   pre_off[i+1]), then for every column ',"0.0"' for a zero and ',"<n>"' (is_int[i] != 0) or ',"<n>.0"' otherwise,
   then a newline.  Returns once the block's size is known (*bytes_out); the text itself is rendered and copied to a
   pinned host buffer behind it.  The host buffer of the slot must no longer be in use (scape_hip_report_fetch). */
int scape_hip_report_render(scape_hip_ctx *ctx, int32_t slot, int32_t n_rows, const int64_t *rows, const int8_t *is_int,
                            const int64_t *pre_off, const char *pre, int64_t *bytes_out);
/* Render the same rows as Matrix Market coordinate entries into slot 0 or 1: row i is number row_no0 + i of the file
   (row_no0 >= 1), and each of its nonzero columns c, ascending, gives the line "<row_no0 + i> <c + 1> <count>\n".
   *bytes_out = the block's text bytes, *nnz_out = its entries; the rest as scape_hip_report_render. */
int scape_hip_report_render_mtx(scape_hip_ctx *ctx, int32_t slot, int32_t n_rows, const int64_t *rows, int64_t row_no0,
                                int64_t *bytes_out, int64_t *nnz_out);
/* ex_pa_len_mat: render the expected pA length of every (record, column) with reads as Matrix Market entries into slot
   0 or 1.  Record i of the block owns the count rows rec_row0[i] .. rec_row0[i] + K[i] - 1 of the last counts call and
   is row row_no0 + i of the file (row_no0 >= 1).  For each of its columns c, ascending, with T = the sum of the K counts
   above 0 it gives the line "<row_no0 + i> <c + 1> <field>\n"; a record with skip[i] != 0 gives none.  The field is
     what == 1: T;
     what == 0: '%.6f' of v, the reference's exp_pa_len (apa_core.py:1038-1052) of that cell's reads: v = 1.0 when
       K[i] == 1, otherwise the sum over l of (c_l / T) * n_l with n_l = n_arr[n_off[i] + l], every operation a correctly
       rounded f64 one without contraction, the sum in the order of numpy's pairwise sum (below 8 terms sequentially from
       0.0; up to 128 terms eight accumulators over the multiples of 8, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the
       remainder sequentially; above that the first n/2 terms rounded down to a multiple of 8 plus the rest, recursively),
       then added to 0.0.  The text is exact: with v = +-m 2^e, m 10^6 2^e is rounded half to even to an integer q and
       printed as the sign bit's '-', the digits of q / 10^6, '.', and the six digits of q % 10^6.  The caller keeps
       |n_l| < 2^31 / 9 and every n_l finite for the records it does not skip (n_arr is not read for the skipped ones).
   *bytes_out = the block's text bytes (0 when no record of the block has an entry; the slot is then fetched as 0 bytes),
   *nnz_out = its entries; the rest as scape_hip_report_render. */
int scape_hip_report_render_len_mtx(scape_hip_ctx *ctx, int32_t slot, int32_t n_rec, const int64_t *rec_row0,
                                    const int32_t *K, const int64_t *n_off, const double *n_arr, const int8_t *skip,
                                    int64_t row_no0, int32_t what, int64_t *bytes_out, int64_t *nnz_out);
/* ex_pa_usage_mat (report_mtx.inc): the per-cell usage c_l / T of every pA site.  scape_hip_report_usage_totals forms, for
   n_rec records of the last counts call (record i owns the count rows rec_row0[i] .. rec_row0[i] + K[i] - 1) and every
   column c, T[i][c] = the sum of the K[i] counts of column c (int32: a record holds at most INT32_MAX reads), and keeps
   them on the device beside the counts until the next scape_hip_report_counts, scape_hip_report_usage_totals or
   scape_hip_report_free call.  It returns once the kernel is queued. */
int scape_hip_report_usage_totals(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *rec_row0, const int32_t *K);
/* Render n_rows rows as Matrix Market entries into slot 0 or 1.  Row i is count row rows[i] of the last counts call, one
   of the rows of record row_rec[i] of the last totals call, and is row row_no0 + i of the file (row_no0 >= 1).  With c
   its count and T its record's total in a column, each column, ascending, gives the line
   "<row_no0 + i> <column + 1> <field>\n" where
     what == 0: c > 0 and T >= min_reads; the field is '%.6f' of the double (double)c / (double)T, one correctly rounded
       f64 division, printed exactly as scape_hip_report_render_len_mtx prints its values (ties to even on the binary
       value: 1 / 128 is 0.007812);
     what == 1: T >= min_reads, whatever c is; the field is T.
   min_reads >= 1.  *bytes_out = the block's text bytes (0 when no row of the block has an entry; the slot is then
   fetched as 0 bytes), *nnz_out = its entries; the rest as scape_hip_report_render.  An error return (no counts, no
   totals since the last counts, a slot or `what` outside 0 / 1, min_reads < 1, a row or record index out of range, a
   row outside its record) leaves *bytes_out and *nnz_out as they were. */
int scape_hip_report_render_usage_mtx(scape_hip_ctx *ctx, int32_t slot, int32_t n_rows, const int64_t *rows,
                                      const int32_t *row_rec, int64_t row_no0, int32_t min_reads, int32_t what,
                                      int64_t *bytes_out, int64_t *nnz_out);
/* Pseudo-bulk sums of the last counts call (ex_pa_pseudobulk): segment s is the columns [seg_off[s], seg_off[s+1]) of
   the count matrix, 0 <= seg_off[0] <= ... <= seg_off[n_seg] <= n_cols (the caller passes scape_hip_report_counts an
   id2col that puts every sample's columns side by side).  For row i (count row rows[i]) and segment s,
   sum_out[i * n_seg + s] is the sum of the counts and nz_out[i * n_seg + s] the number of counts above 0.  Returns
   once both arrays are on the host. */
int scape_hip_report_group_sums(scape_hip_ctx *ctx, int32_t n_seg, const int32_t *seg_off, int32_t n_rows,
                                const int64_t *rows, int32_t *sum_out, int32_t *nz_out);
/* The permutation tests (perm.inc).
   diff_pa: permutation test of pA usage between two cell populations.  The tested columns are the first n = n1 + n2
   columns of the count matrix (the caller passes scape_hip_report_counts an id2col that puts population 1's columns
   first, then population 2's); position j = column j.  Permutation 0 is the observed labelling (positions < n1).
   Permutation p >= 1 gives population 1 the n1 positions with the smallest key(p, j), all arithmetic mod 2^64:
     G = 0x9E3779B97F4A7C15
     mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)
     h(p, j) = mix(mix(seed + G * p) + G * (j + 1)),  key(p, j) = (h(p, j) & ~0xFFFFFF) | j
   scape_hip_report_perm_masks builds the membership bits of permutations p_first .. p_first + p_count - 1 (p_first >= 1)
   on the device, p_count * ceil(n / 64) * 8 bytes laid out [column word][permutation]; they replace the bits of an
   earlier call and stay until scape_hip_report_free, across scape_hip_report_counts calls.  n1, n2 >= 1, n < 2^24.
   The call is scape_hip_report_perm_masks_strata's with one stratum of every cell, p_count * 8 bytes of scratch included. */
int scape_hip_report_perm_masks(scape_hip_ctx *ctx, int32_t n1, int32_t n2, int64_t p_first, int32_t p_count,
                                uint64_t seed);
/* Labellings permuted within strata only (blocked permutations: cell type, donor, batch, ...).  Positions: population 1's
   columns first, then population 2's, as above; within each population the columns are ordered by stratum.  Stratum s
   of n_strata has m1[s] cells in population 1 and m2[s] in population 2 and so owns the position ranges
     [o1[s], o1[s] + m1[s])  and  [n1 + o2[s], n1 + o2[s] + m2[s]),   o1 / o2 = the exclusive prefix sums of m1 / m2,
   n1 = sum m1, n2 = sum m2, n = n1 + n2 < 2^24.  Permutation 0 is the observed labelling (positions < n1).  Permutation
   p >= 1 gives population 1, in every stratum separately, the m1[s] positions of that stratum with the smallest
   key(p, j) - the key above, unchanged, with j the global position, so keys are distinct.  Exactly m1[s] bits are set
   per stratum, also when m1[s] = 0 or m2[s] = 0: such a stratum's cells never move but are still counted.  With one
   stratum the bits are those of scape_hip_report_perm_masks, bit for bit.
   The call fills the same buffer in the same layout and takes the place of a scape_hip_report_perm_masks call:
   scape_hip_report_perm_test and scape_hip_report_perm_len run behind either.  It also holds p_count * n_strata * 8
   bytes of scratch on the device.  Checked before anything is queued: n_strata >= 1, every m1[s], m2[s] >= 0 and
   m1[s] + m2[s] >= 1, n1, n2 >= 1, n < 2^24, p_first, p_count >= 1. */
int scape_hip_report_perm_masks_strata(scape_hip_ctx *ctx, int32_t n_strata, const int32_t *m1, const int32_t *m2,
                                       int64_t p_first, int32_t p_count, uint64_t seed);
/* The ceil(n / 64) membership words of permutation p_first + p (0 <= p < p_count) of the last masks call, whichever of
   the two entry points made it: bit j % 64 of words_out[j / 64] is set when position j is in population 1. */
int scape_hip_report_perm_bits_get(scape_hip_ctx *ctx, int32_t p, uint64_t *words_out);
/* The test of n_rec records of the last counts call against the permutations of the last perm_masks call.  Record r owns
   the kept count rows rows[rec_row_off[r] .. rec_row_off[r+1]) (rec_row_off[0] = 0, non-decreasing).  Per row i:
   t_out[i] = its sum over the tested columns, a0_out[i] = its sum over population 1 as observed.  With T, A, B the
   record's sums of t, a and t - a under a labelling, N_i = a_i T - t_i A (64-bit integers),
     S = sum_i N_i^2 / (t_i A B)   and   d_i = N_i / (A B)      (both 0 when A = 0 or B = 0), in f64, rows in order.
   stat0_out[r] = S of the observed labelling.  The call ADDS to site_n_ge_out[i] the number of its permutations with
   |d_i(p)| >= |d_i(0)| (1 - 2^-40) and to gene_n_ge_out[r] those with S(p) >= S(0) (1 - 2^-40): the caller zeroes both
   arrays before the first chunk of permutations and passes them again for every further chunk (the device counters
   themselves start at zero in every call, and S(0), d_i(0) are formed anew, so chunks do not depend on each other). */
int scape_hip_report_perm_test(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                               int64_t *t_out, int64_t *a0_out, int64_t *site_n_ge_out, double *stat0_out,
                               int64_t *gene_n_ge_out);
/* diff_pa_len: permutation test of a record's mean pA position between the two populations, on the counts call, the
   masks call, the kept rows and the labellings of scape_hip_report_perm_test (same seed = same labellings).  Kept row i
   carries the weight w[i] = x_i - min x over its record's rows, x_i the row's position (alpha_arr[label], f64: larger =
   more distal = longer 3'UTR), so 0 <= w[i] <= span = max x - min x; tol[r] = 2^-40 * span of record r.  Under a
   labelling with row sums a_i over population 1 and b_i = t_i - a_i (formed as an integer), A = sum a_i, B = sum b_i,
   the device forms in f64, contraction off, rows in order,
     W1 = sum_i (double)a_i * w_i,  W2 = sum_i (double)b_i * w_i,  delta = W1 / A - W2 / B   (0 when A = 0 or B = 0)
   through one device function for the observed labelling and every permutation; delta = mean_pos.1 - mean_pos.2 (the
   shift by min x cancels), > 0 when population 1's reads end further out.  delta0_out[r] = delta of the observed
   labelling, t_out / a0_out as for perm_test.  The call ADDS to n_ge_out[r] the number of its permutations with
   |delta(p)| >= |delta(0)| - tol[r] (two-sided; the caller zeroes the array before the first chunk of permutations).
   Each mean is within (R + 1) 2^-53 span of its exact value for R rows, delta within (2 R + 3) 2^-53 span, and a
   record may own at most 1,024 rows (checked), so the observed and a permuted |delta| and the threshold's subtraction
   are together off by at most 4,103 * 2^-53 span, about half of tol: a labelling whose exact |delta| reaches the observed
   one is always counted, one more than 2 tol below it never (derivation: csrc/perm.inc above k_rep_perm_len).  The
   band is absolute, not relative as in perm_test, because delta is a difference of two means and can cancel.
   w and tol must be finite and not negative. */
int scape_hip_report_perm_len(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                              const double *w, const double *tol, int64_t *t_out, int64_t *a0_out, double *delta0_out,
                              int64_t *n_ge_out);
/* diff_pa_groups: the omnibus form of the permutation test, for G = n_groups populations (2 <= G <= 64) of
   sizes[g] >= 1 cells, n = sum sizes < 2^24.  The tested columns are the first n columns of the count matrix, population
   0's first, then population 1's, ...; position j = column j.  Permutation 0 is the observed labelling (group = the
   population of the position).  Permutation p >= 1 ranks the n keys key(p, j) - the key of scape_hip_report_perm_masks,
   unchanged, so keys are distinct - and gives position j of rank r(p, j) the group
     g(p, j) = #{h in 1 .. G-1 : c_h <= r(p, j)},   c_h = sizes[0] + .. + sizes[h-1]:
   the sizes[0] smallest keys form group 0, the next sizes[1] group 1, and so on.  With G = 2, group 0 is population 1
   of scape_hip_report_perm_masks(n1 = sizes[0], n2 = sizes[1]) for the same seed, position for position.
   scape_hip_report_perm_labels builds the groups of permutations p_first .. p_first + p_count - 1 on the device, one byte
   per (position, permutation): p_count * n bytes laid out [position][permutation] (the G - 1 cut keys of a permutation
   live in LDS only).  They replace the labels of an earlier call and stay until scape_hip_report_free, across
   scape_hip_report_counts calls; the membership bits of scape_hip_report_perm_masks are a separate buffer.  Checked
   before anything is queued: 2 <= n_groups <= 64, every size >= 1, n < 2^24, p_first >= 1, p_count >= 1. */
int scape_hip_report_perm_labels(scape_hip_ctx *ctx, int32_t n_groups, const int32_t *sizes, int64_t p_first,
                                 int32_t p_count, uint64_t seed);
/* The n groups of permutation p_first + p (0 <= p < p_count) of the last labels call: labels_out[j] = g(p_first + p, j). */
int scape_hip_report_perm_labels_get(scape_hip_ctx *ctx, int32_t p, uint8_t *labels_out);
/* The test of n_rec records of the last counts call against the permutations of the last perm_labels call; records, kept
   rows and the ADD semantics as in scape_hip_report_perm_test.  n_groups and seg_off[n_groups + 1] name the groups'
   column ranges as observed: seg_off[0] = 0 and seg_off[g + 1] - seg_off[g] = sizes[g] of the labels call (checked).
   Per row i: t_out[i] = its sum over the tested columns, a0_out[i * n_groups + g] = its sum over group g as observed.
   Under a labelling with row sums a_ig, A_g = sum_i a_ig, T = sum_i t_i < 2^31 (checked) and the 64-bit integer
   N_ig = a_ig T - t_i A_g, the device forms in f64, contraction off, groups and rows in order,
     s_i = sum_{g : A_g > 0} N_ig^2 / A_g      and      S = sum_i s_i / (T t_i)
   (S is Pearson's chi-square of the rows x G table; for G = 2 it equals perm_test's sum N_i^2 / (t_i A B) as a rational;
   s_i is proportional, by factors that do not depend on the labelling, to the chi-square of the 2 x G table "row i
   against the record's other rows") through one device function for the observed labelling and every permutation.
   stat0_out[r] = S(0), site_stat0_out[i] = s_i(0) / (T t_i), the row's share of it.  The call ADDS to site_n_ge_out[i]
   the number of its permutations with s_i(p) >= s_i(0) (1 - 2^-40) and to gene_n_ge_out[r] those with
   S(p) >= S(0) (1 - 2^-40); the caller zeroes both before the first chunk of permutations.
   Rounding: every term is positive and the sums are nested (groups within a row, rows within the record), so S of a
   record of R rows is within (R + G + 4) 2^-53 of its rational, relatively - the error grows with R + G, not with R x G.
   Two equal rationals always tie inside the 2^-40 slack, and a labelling at S(0) (1 - 2^-39) or below is never counted,
   when 2 (R + G + 4) + 1 < 2^13; a record with R + G > 4,000 is refused ("record <r>: ..."), which leaves 183 * 2^-53
   to spare (derivation: csrc/perm.inc, section "G-way labellings").  s_i is within (G + 3) 2^-53 for any R.
   LDS: 2 * n_groups KiB per workgroup of 256 permutations. */
int scape_hip_report_perm_groups(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                 int32_t n_groups, const int32_t *seg_off, int64_t *t_out, int64_t *a0_out,
                                 int64_t *site_n_ge_out, double *stat0_out, double *site_stat0_out,
                                 int64_t *gene_n_ge_out);
/* diff_pa_len_groups: the omnibus form of scape_hip_report_perm_len, on the counts call, the labels call, the kept rows
   and the ADD semantics of scape_hip_report_perm_groups (n_groups / seg_off checked against the labels call in the same
   way; same seed = same labellings).  Kept row i carries the INTEGER position q[i], 0 <= q[i] <= 2^22 (checked): the
   caller scales x_i - min x of the record by the power of two that puts qspan = max q into 2^21 .. 2^22 and rounds.
   tol_stat[r] = 2^-40 T qspan^2 and tol_delta[r] = 2^-40 qspan of record r (finite, not negative: checked).  Under a
   labelling with a_ig the sum of row i over group g, the device forms the exact integers
     A_g = sum_i a_ig,   Q_g = sum_i a_ig q_i   (32- and 64-bit LDS adds, any order),   T = sum_g A_g < 2^31 (checked),
     Q = sum_g Q_g <= 2^53
   and from them in f64, contraction off, through one pair of device functions for the observed labelling and every
   permutation, with m = (double)Q / (double)T formed once per record,
     D   = sum_{g : A_g > 0} A_g (Q_g / A_g - m)^2            (groups in order)
     d_g = Q_g / A_g - (Q - Q_g) / (T - A_g)                  (0 when A_g = 0 or A_g = T).
   D is the between-group sum of squares of the position weighted by reads (as a rational sum Q_g^2 / A_g - Q^2 / T; for
   G = 2 it is (A_0 A_1 / T) d_0^2), d_g the mean position of group g against that of all the others.  t_out[i] and
   a0_out[i * n_groups + g] as for perm_groups; stat0_out[r] = D(0), delta0_out[r * n_groups + g] = d_g(0).  The call
   ADDS to n_ge_out[r] the number of its permutations with D(p) >= D(0) - tol_stat[r] and to
   group_n_ge_out[r * n_groups + g] those with |d_g(p)| >= |d_g(0)| - tol_delta[r] (two-sided; for a group whose observed
   A_g is 0 or T, d_g(0) = 0 and every permutation counts: the caller reports no test for it).
   Rounding (u = 2^-53): every integer converted is below 2^53, so nothing depends on the number of rows or nonzeros.  Each
   mean is within u qspan, the difference Q_g / A_g - m within 3 u qspan, a term of D within A_g (6 u qspan |e| + 2 u e^2),
   all terms within 8 u T qspan^2, and the G - 1 roundings of the sum add (G - 1) u T qspan^2:
     |D - exact| <= (G + 8) u T qspan^2,     |d_g - exact| <= 3 u qspan.
   Observed value, permuted value and the threshold's own subtraction are together off by at most (2 G + 17) u T qspan^2
   <= 145 u T qspan^2 and 7 u qspan, against bands of 2^-40 = 8,192 u: a labelling whose exact statistic reaches the
   observed one is always counted, one more than twice the band below it never (derivation: csrc/perm.inc, section
   "diff_pa_len_groups").  No cap beyond G <= 64, q <= 2^22 and T < 2^31 is needed.
   LDS: 12 bytes per lane and group, 3 KiB per group; above 32 groups they are taken in equal slices of at most 32 (96
   KiB), one walk over the record's nonzeros per slice, with the same result whatever the slice. */
int scape_hip_report_perm_len_groups(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                     int32_t n_groups, const int32_t *seg_off, const int32_t *q, const double *tol_stat,
                                     const double *tol_delta, int64_t *t_out, int64_t *a0_out, double *stat0_out,
                                     double *delta0_out, int64_t *n_ge_out, int64_t *group_n_ge_out);
/* diff_pa_pairs: every pair of G = n_groups populations (2 <= G <= 64, sizes[g] >= 1 cells) tested as diff_pa tests two,
   from one counts call.  The populations sit in the column segments seg_off in front of the count matrix, population 0's
   columns first, as for scape_hip_report_perm_labels.  Pair k of n_pairs (1 .. 2016) is (pair_g[k], pair_h[k]),
   0 <= g < h < G, population g against population h.  Its local positions are 0 .. sizes[g] - 1 for g's columns in order
   and sizes[g] .. sizes[g] + sizes[h] - 1 for h's; permutation p >= 1 gives g the sizes[g] local positions with the
   smallest key(p, local position), the key above, unchanged: the bits of pair k are those of
   scape_hip_report_perm_masks(sizes[g], sizes[h], p_first, p_count, seed), bit for bit.
   scape_hip_report_perm_pair_masks builds them for permutations p_first .. p_first + p_count - 1 on the device: per
   pair ceil((sizes[g] + sizes[h]) / 64) words per permutation, laid out [pair's word offset + word][permutation], and one
   8-byte key bound per (pair, permutation).  They are a buffer of their own, replace those of an earlier call and stay
   until scape_hip_report_free.  Checked before anything is queued or released: 2 <= n_groups <= 64, every size >= 1,
   1 <= n_pairs <= 2016, every pair 0 <= g < h < n_groups with fewer than 2^24 cells, p_first >= 1, p_count >= 1, fewer
   than 2^31 words over all pairs; a call refused by a check keeps the earlier bits. */
int scape_hip_report_perm_pair_masks(scape_hip_ctx *ctx, int32_t n_groups, const int32_t *sizes, int32_t n_pairs,
                                     const int32_t *pair_g, const int32_t *pair_h, int64_t p_first, int32_t p_count,
                                     uint64_t seed);
/* The membership words of pair `pair` under permutation p_first + p (0 <= p < p_count) of the last pair masks call: bit
   j % 64 of words_out[j / 64] is set when local position j is in the pair's first population. */
int scape_hip_report_perm_pair_bits_get(scape_hip_ctx *ctx, int32_t pair, int32_t p, uint64_t *words_out);
/* The test of n_rec records of the last counts call by the pairs pair_first .. pair_first + pair_count - 1 of the last
   pair masks call; records, kept rows and the ADD semantics as in scape_hip_report_perm_test, n_groups / seg_off checked
   against the pair masks call as scape_hip_report_perm_groups checks them against the labels call.  The rows are those
   kept over ALL groups.  t_out[i] = the row's sum over the tested columns, a0_out[i * n_groups + g] = its sum over group
   g, so for pair (g, h) t_i = a0[i][g] + a0[i][h].  The pair tests record r when at least two of its rows have t_i > 0
   and both populations have reads; then, over the rows with t_i > 0 in order, S and d_i are those of
   scape_hip_report_perm_test (one device function, contraction off, the same 1 - 2^-40 slack; a row with t_i = 0 adds
   exactly 0.0), so stat0_out[k * n_rec + r] has the bits, and site_n_ge_out[k * n_rows + i] (ADDED to; rows with t_i = 0
   are left alone) and gene_n_ge_out[k * n_rec + r] (ADDED to) the values, of a scape_hip_report_perm_test call on the
   pair's own two populations, k counting from pair_first.  For a record the pair does not test stat0_out is 0 and nothing
   is added.  pair_count * n_rec < 2^31.
   LDS: 1 KiB per row of a record held at once, in the classes 4 .. 64 rows of scape_hip_report_perm_test. */
int scape_hip_report_perm_pairs(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                int32_t n_groups, const int32_t *seg_off, int32_t pair_first, int32_t pair_count,
                                int64_t *t_out, int64_t *a0_out, int64_t *site_n_ge_out, double *stat0_out,
                                int64_t *gene_n_ge_out);
/* diff_pa_markers: each of n_markers populations (1 .. 64, sizes[g] >= 1 cells) tested, as diff_pa tests two, against ALL
   other tested cells, from one counts call.  The tested columns are the first n = sum sizes + n_others columns of the
   count matrix: marker 0's columns first, then marker 1's, ..., then a segment of n_others >= 0 "others" (tested cells of
   no marker); slot j is that position.  orig_rank[j] is the rank of slot j's column among the n tested columns in the
   caller's own column order, a permutation of 0 .. n - 1 that ascends within every segment.  Marker g is
   scape_hip_report_perm_masks(sizes[g], n - sizes[g], p_first, p_count, seed) on the layout that puts g's columns first
   and every other tested column behind them in the caller's order: slot j has the local position
     local_g(j) = j - (sizes[0] + .. + sizes[g-1])                                  in g's own segment,
     local_g(j) = sizes[g] + orig_rank[j] - #{cells of g with a smaller orig_rank}    anywhere else,
   and permutation p >= 1 gives g the sizes[g] local positions with the smallest key(p, local position), the key above,
   unchanged.  scape_hip_report_perm_marker_masks builds the bits of permutations p_first .. p_first + p_count - 1 on the
   device IN SLOT ORDER: ceil(n / 64) words per marker and permutation, laid out [marker * words + word][permutation], and
   one 8-byte key bound per (marker, permutation); local_g is found by a search in g's ranks, no table is kept.  They are
   a buffer of their own, replace those of an earlier call and stay until scape_hip_report_free.  Checked before anything
   is queued or released: 1 <= n_markers <= 64, every size >= 1, n_others >= 0, 2 <= n < 2^24, every marker smaller than
   n, orig_rank as stated, p_first >= 1, p_count >= 1, fewer than 2^31 words over all markers; a call refused by a check
   keeps the earlier bits. */
int scape_hip_report_perm_marker_masks(scape_hip_ctx *ctx, int32_t n_markers, const int32_t *sizes, int32_t n_others,
                                       const int32_t *orig_rank, int64_t p_first, int32_t p_count, uint64_t seed);
/* The ceil(n / 64) membership words of marker `marker` under permutation p_first + p (0 <= p < p_count) of the last
   marker masks call: bit j % 64 of words_out[j / 64] is set when SLOT j is in the marker's population. */
int scape_hip_report_perm_marker_bits_get(scape_hip_ctx *ctx, int32_t marker, int32_t p, uint64_t *words_out);
/* The test of n_rec records of the last counts call by the markers marker_first .. marker_first + marker_count - 1 of the
   last marker masks call; records, kept rows and the ADD semantics as in scape_hip_report_perm_test.  n_seg = n_markers
   + 1 and seg_off[n_seg + 1] name the column ranges of the markers and of the others (the last segment, which may be
   empty), checked against the marker masks call as scape_hip_report_perm_groups checks its groups.  t_out[i] = the row's
   sum over the n tested columns, a0_out[i * n_seg + g] = its sum over segment g: t_i and T are the same for every
   marker.  Marker g tests record r when at least two of its rows have t_i > 0 and 0 < A_g(0) < T; then S and d_i are those
   of scape_hip_report_perm_test (one device function, contraction off, the same 1 - 2^-40 slack, rows in order), so
   stat0_out[k * n_rec + r] has the bits, and site_n_ge_out[k * n_rows + i] and gene_n_ge_out[k * n_rec + r] (both ADDED
   to) the values, of a scape_hip_report_perm_test call on the marker's population against all other tested cells, k
   counting from marker_first.  For a record the marker does not test stat0_out is 0 and nothing is added.
   marker_count * n_rec < 2^31.
   LDS: 1 KiB per row of a record held at once, in the classes 4 .. 64 rows of scape_hip_report_perm_test. */
int scape_hip_report_perm_markers(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                  int32_t n_seg, const int32_t *seg_off, int32_t marker_first, int32_t marker_count,
                                  int64_t *t_out, int64_t *a0_out, int64_t *site_n_ge_out, double *stat0_out,
                                  int64_t *gene_n_ge_out);
/* diff_pa_len_pairs: every pair of the last pair masks call tested as scape_hip_report_perm_len tests two populations,
   from the counts call, the bits and the one compaction of scape_hip_report_perm_pairs.  (ABI 4 gains this entry point
   and the next; nothing that was there changes.)  Records, kept rows (those kept
   over ALL groups), the range pair_first / pair_count, t_out and a0_out [row][group], the checks of n_groups / seg_off
   and of the range, and the ADD semantics are those of that call.  x[i] is the pA position of kept row i (alpha_arr[label],
   f64, NOT yet shifted).  Pair (g, h) owns the rows of a record with t_i = a0[i][g] + a0[i][h] > 0 and tests the record
   when two such rows or more remain, both populations have reads and span = max x - min x over THOSE rows is > 0.  Then
   the device forms, over those rows in order, w_i = x_i - min x (one f64 subtraction) and tol = 2^-40 span, and W1, W2
   and delta through the device functions of scape_hip_report_perm_len, contraction off.  A row without a read in the
   pair is passed over, not multiplied by 0: its w would lie outside 0 .. span.  So delta0_out[k * n_rec + r] has the
   bits, and n_ge_out[k * n_rec + r] (ADDED to: the permutations with |delta(p)| >= |delta(0)| - tol) the value, of a
   scape_hip_report_perm_len call behind scape_hip_report_perm_masks on the pair's own two populations and rows, k
   counting from pair_first.  For a record the pair does not test delta0_out is 0.0 and nothing is added.  The rounding
   bound of scape_hip_report_perm_len holds: a pair's rows are a subset of the record's, of which there may be at most
   1,024.  Checked before anything is queued, beside the checks of scape_hip_report_perm_pairs: x and the outputs are
   there, every x is finite and so is max x - min x of every record, no record owns more than 1,024 rows; a refused call
   leaves masks and counts in place.  pair_count * n_rec < 2^31.  No LDS: any number of rows in one launch. */
int scape_hip_report_perm_len_pairs(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                    int32_t n_groups, const int32_t *seg_off, int32_t pair_first, int32_t pair_count,
                                    const double *x, int64_t *t_out, int64_t *a0_out, double *delta0_out,
                                    int64_t *n_ge_out);
/* diff_pa_len_markers: every marker of the last marker masks call tested as scape_hip_report_perm_len tests a population
   against all other tested cells, from the counts call, the bits (in slot order) and the one compaction of
   scape_hip_report_perm_markers; records, kept rows, the range marker_first / marker_count, n_seg / seg_off and their
   checks, t_out and a0_out [row][segment] and the ADD semantics are those of that call, x and its checks those of
   scape_hip_report_perm_len_pairs.  The kept rows with t_i > 0, min x, w_i and tol = 2^-40 span are the same for every
   marker.  Marker g tests record r when two rows or more have t_i > 0, 0 < A_g(0) < T and span > 0; then
   delta0_out[k * n_rec + r] has the bits, and n_ge_out[k * n_rec + r] (ADDED to) the value, of a
   scape_hip_report_perm_len call on the marker's population against all other tested cells, k counting from
   marker_first; otherwise delta0_out is 0.0 and nothing is added.  marker_count * n_rec < 2^31.  No LDS. */
int scape_hip_report_perm_len_markers(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                      int32_t n_seg, const int32_t *seg_off, int32_t marker_first, int32_t marker_count,
                                      const double *x, int64_t *t_out, int64_t *a0_out, double *delta0_out,
                                      int64_t *n_ge_out);
/* diff_pa_trend: the test of pA usage ALONG an integer score of the cells, on the keys of scape_hip_report_perm_masks.
   (ABI 4 gains the three entry points below; nothing that was there changes.)  The tested columns are the first n
   columns of the count matrix, position j = column j, 2 <= n < 2^24; q[j] is the observed score of position j, 0 <= q[j]
   <= 32,768.  Permutation 0 is the observed assignment.  Permutation p >= 1 ranks the positions by the unchanged key(p, j)
   - rho_p(j) = #{i : key(p, i) < key(p, j)}, a bijection because keys are distinct - and position j receives the score
     z_p(j) = q[rho_p(j)].
   When q[j] is the group index of column segments (non-decreasing in j), z_p(j) is the byte that
   scape_hip_report_perm_labels writes for the same sizes and seed.  The call builds the scores of permutations
   p_first .. p_first + p_count - 1 on the device, a halfword per (position, permutation) laid out [position][permutation],
   by ranking EVERY key: per permutation the positions are sorted into buckets of the keys' leading bits (2^10 .. 2^14
   counters in LDS, chosen from n; n int32 of scratch per permutation of the call) and a position's rank is its bucket's
   start plus the number of the bucket's members with a smaller key, a count that does not depend on the order in which
   the members arrived.  6 n bytes per permutation in all.  The scores replace those of an earlier call and stay, with q,
   until scape_hip_report_free.  Checked before anything is queued: n, every q[j], p_first >= 1, p_count >= 1. */
int scape_hip_report_perm_scores(scape_hip_ctx *ctx, int32_t n, const uint16_t *q, int64_t p_first, int32_t p_count,
                                 uint64_t seed);
/* The n scores of permutation p_first + p (0 <= p < p_count) of the last scores call: scores_out[j] = z(p_first + p, j). */
int scape_hip_report_perm_scores_get(scape_hip_ctx *ctx, int32_t p, uint16_t *scores_out);
/* The test of n_rec records of the last counts call against the permutations of the last perm_scores call; records, kept
   rows and the ADD semantics as in scape_hip_report_perm_test.  With c_ij the count of kept row i at position j, under
   scores z the device forms the exact integers
     t_i = sum_j c_ij,   T = sum_i t_i < 2^31 (checked),   s_i = sum_j c_ij z(j) < 2^46,   S = sum_i s_i
   (64-bit registers; S first, in a walk over all the record's nonzeros, then s_i row by row) and from them in f64,
   contraction off, through the pair of device functions of scape_hip_report_perm_len_groups for the observed scores and
   every permutation, with m = (double)S / (double)T formed once per labelling,
     D   = sum_i t_i (s_i / t_i - m)^2                    (rows in order)
     d_i = s_i / t_i - (S - s_i) / (T - t_i).
   D is the between-site sum of squares of the score over the record's reads (as a rational sum s_i^2 / t_i - S^2 / T),
   d_i the mean score of site i's reads against that of the record's other reads.  t_out[i], s0_out[i] = s_i(0) and
   sq0_out[i] = sum_j c_ij q_j^2 (below 2^61) per kept row, d0_out[i] = d_i(0), stat0_out[r] = D(0).  The call ADDS to
   site_n_ge_out[i] the number of its permutations with |d_i(p)| >= |d_i(0)| - 2^-40 qspan (two-sided; qspan = max q of the
   scores call) and to gene_n_ge_out[r] those with D(p) >= D(0) - 2^-40 T qspan^2; the caller zeroes both before the
   first chunk of permutations.
   Rounding (u = 2^-53): the analysis of scape_hip_report_perm_len_groups with the kept rows in the place of the groups,
     |D - exact| <= (R + 8) u T qspan^2,     |d_i - exact| <= 3 u qspan     for a record of R rows.
   Observed value, permuted value and the threshold's own subtraction are together off by at most (2 R + 17) u T qspan^2,
   which stays below the band of 2^-40 = 8,192 u for R <= 4,000: a record with more kept rows is refused ("record <r>:
   ..."), which leaves 175 u to spare; then a labelling whose exact statistic reaches the observed one is always counted,
   one more than twice the band below it never (derivation: csrc/perm.inc, section "diff_pa_trend").  No LDS. */
int scape_hip_report_perm_trend(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                int64_t *t_out, int64_t *s0_out, int64_t *sq0_out, int64_t *site_n_ge_out,
                                double *d0_out, double *stat0_out, int64_t *gene_n_ge_out);
/* diff_pa_len_trend: the test of the pA POSITION (3'UTR length) along the scores, for n_rec records of the last counts
   call against the permutations of the last perm_scores call; records, kept rows and the ADD semantics as in
   scape_hip_report_perm_trend.  (ABI 4 gains this entry point; nothing that was there changes.)  x[i] is the integer
   position of kept row i, 0 <= x[i] <= 2^22.  With c_ij the count of kept row i at position j, under scores z the device
   forms the exact integers
     t_i = sum_j c_ij,   T = sum_i t_i < 2^31,   Sx = sum_i t_i x_i                               (fixed)
     s_i = sum_j c_ij z(j) < 2^46,   Sz = sum_i s_i < 2^46,   Sxz = sum_i x_i s_i < 2^63          (per labelling)
     C   = T Sxz - Sx Sz
   in signed 64-bit registers and, for C, as two 64 x 64 -> 128-bit products (each below 2^94) and their difference.  C
   is T^2 times the covariance of position and score over the record's reads; T, Sx and sum_i t_i x_i^2 are the same
   under every labelling, so |C| orders the labellings as the absolute slope of the score regressed on the position
   does.  t_out[i], s0_out[i] = s_i(0) and sq0_out[i] = sum_j c_ij q_j^2 (below 2^61) per kept row; c0_out[2 r] and
   c0_out[2 r + 1] = the low and the high 64 bits of the two's-complement C(0).  The call ADDS to n_ge_out[r] the number
   of its permutations with |C(p)| >= |C(0)| (two-sided), compared as 128-bit integers: there is no rounding, no band
   and no bound on a record's rows; the caller zeroes n_ge_out before the first chunk of permutations.
   Checked before anything is queued: a scores call exists, the offsets and rows, every x[i].  T comes from the device,
   so the two checks on it are made per record ("record <r>: ...") once the row sums are back - t_out is written by
   then, and for the second the compaction of the rows is queued - and before the test's own kernels are queued: T <
   2^31, and T max_i x_i < 2^48, which with scores of at most 2^15 keeps Sxz below 2^63 and Sx below 2^48.  No LDS, no
   f64, no division. */
int scape_hip_report_perm_len_trend(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                    const int32_t *x, int64_t *t_out, int64_t *s0_out, int64_t *sq0_out,
                                    int64_t *c0_out /* [2 r] low, [2 r + 1] high 64 bits of C(0) */,
                                    int64_t *n_ge_out /* ADDED to */);
/* boot_pa_len: the cell bootstrap of a record's mean pA position in each of G = n_groups populations (1 <= G <= 64).
   (ABI 4 gains these five entry points; nothing that was there changes.)  The tested columns are the first n columns
   of the count matrix, population 0's first, then population 1's, ...; position j = column j, and cell[j] >= 0 is the
   0-based column that the cell of position j has in ex_pa_cnt_mat's matrix.  The hash sees cell[j], not j, so a cell's
   multiplicity depends on the seed, the replicate and the cell only, never on the clustering.  All arithmetic mod 2^64,
   G and mix those of scape_hip_report_perm_masks:
     h(b, c) = mix(mix(seed + G * b) + G * (c + 1)),  all 64 bits
     m(b, c) = #{k in 0..14 : h(b, c) >= P[k]}  for replicate b >= 1 (0 <= m <= 15);  replicate 0 is the observed data, m = 1
     P[k] = floor(2^64 * e^-1 * sum_{i <= k} 1 / i!):
       0x5E2D58D8B3BCDF1A 0xBC5AB1B16779BE35 0xEB715E1DC1582DC2 0xFB23979734A252F1 0xFF1025F59174DC3D
       0xFFD90F3BA4055E19 0xFFFA8B71FC72C913 0xFFFF540C0914B3C9 0xFFFFED1F4AA8F120 0xFFFFFE216E641462
       0xFFFFFFD4D85D3183 0xFFFFFFFC6DA262B4 0xFFFFFFFFBA12D178 0xFFFFFFFFFB07C64C 0xFFFFFFFFFFAB8EA5
   so m is Poisson(1) with the tail beyond 15 (probability 1.9e-14) folded into m = 15.
   scape_hip_report_boot_mult builds m for the replicates b_first .. b_first + b_count - 1 on the device, one byte per
   (position, replicate): b_count * n bytes laid out [position][replicate].  The buffer is its own: the membership bits
   and the labels of the permutation tests are untouched.  It replaces the multiplicities of an earlier call and stays
   until scape_hip_report_free, across scape_hip_report_counts calls.  Checked before anything is queued: 1 <= n < 2^24,
   every cell[j] >= 0, b_first >= 1, b_count >= 1.  A refused call of these five names its entry point in the message. */
int scape_hip_report_boot_mult(scape_hip_ctx *ctx, int32_t n, const int32_t *cell, int64_t b_first, int32_t b_count,
                               uint64_t seed);
/* The n multiplicities of replicate b_first + b (0 <= b < b_count) of the last boot_mult call. */
int scape_hip_report_boot_mult_get(scape_hip_ctx *ctx, int32_t b, uint8_t *mult_out);
/* The replicate values of n_rec records of the last counts call under the replicates of the last boot_mult call.
   Records, kept rows, t_out[i] and a0_out[i * n_groups + g] are those of scape_hip_report_perm_len_groups; seg_off[0] =
   0, non-decreasing, seg_off[n_groups] = n of the boot_mult call; q[i] is the INTEGER position of kept row i, 0 <= q[i]
   <= 2^22.  With c_ij the count of kept row i at position j and g(j) the population of position j, the device forms
     A_g(b) = sum_i sum_{j in g} m(b, cell[j]) c_ij,     Q_g(b) = sum_i q_i sum_{j in g} m(b, cell[j]) c_ij
   as exact integers, whatever the order of the adds (a record has T < 2^27 reads in the tested cells, so A <= 15 T <
   2^31 and Q <= 15 T 2^22 < 2^53), and from them
     v_g(b) = (double)Q_g(b) / (double)A_g(b),  one IEEE division, contraction off;  +infinity when A_g(b) = 0.
   Every defined value lies in 0 .. 2^22, so the bit patterns of the values, read as unsigned 64-bit integers, order as
   the values do, with +infinity last.  v_g(b) is stored at column b - 1 of the device-resident f64 array
   vals[r * n_groups + g][n_boot].  A call behind a boot_mult call with b_first = 1 allocates or re-uses the array for
   its record set; a call behind a later chunk of replicates must name the same number of records and groups and the
   same n_boot and fills further columns.  Checked before anything is queued: a counts and a boot_mult call exist, 1 <=
   n_groups <= 64, seg_off, the offsets and rows, every q[i], 1 <= n_boot < 2^31 and the chunk's replicates inside 1 ..
   n_boot.  T comes from the device: a record with T >= 2^27 is refused ("record <r>: ...") once the row sums are back
   and before the kernel of this entry point is queued.  No LDS: a population's sums live in registers. */
int scape_hip_report_boot_len(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                              int32_t n_groups, const int32_t *seg_off, const int32_t *q, int64_t n_boot, int64_t *t_out,
                              int64_t *a0_out);
/* boot_pa_usage: the replicate values of the usage of every kept row (pA site) in every population, under the same
   multiplicities.  (ABI 4 gains this entry point; nothing that was there changes.)  Arguments, t_out, a0_out, the
   checks (without q), the T < 2^27 refusal and the chunk protocol are scape_hip_report_boot_len's.  With c_ij the count
   of kept row i at position j, the device forms
     a_ig(b) = sum_{j in g} m(b, cell[j]) c_ij,     A_g(b) = sum_i a_ig(b) over the kept rows of the row's record
   as exact integers (A <= 15 T < 2^31), and from them
     u_ig(b) = (double)a_ig(b) / (double)A_g(b),  one IEEE division, contraction off;  +infinity when A_g(b) = 0.
   Every defined value lies in 0 .. 1, so the bit patterns order as the values do, with +infinity last.  u_ig(b) is
   stored at column b - 1 of vals[k * n_groups + g][n_boot], k = the index of the kept row in `rows`: the array, its
   written columns and scape_hip_report_boot_vals_get / _boot_quantiles are those of boot_len, and a record set belongs
   to the entry point that began it at replicate 1: a later chunk must name as many rows, the same groups and n_boot and
   come through the same entry point (a boot_usage chunk behind a boot_len record set is refused, and the reverse).
   rows x groups x n_boot x 8 bytes must fit one call.  No LDS, no atomics: a_ig and A_g live in registers; a
   population's nonzeros are walked once for a record of at most 8 kept rows and twice for a longer one. */
int scape_hip_report_boot_usage(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                int32_t n_groups, const int32_t *seg_off, int64_t n_boot, int64_t *t_out,
                                int64_t *a0_out);
/* boot_pa_len_diff and boot_pa_usage_diff: the replicate values of population 0 minus population 1, one series per
   record (len) or per kept row (usage).  (ABI 4 gains these two entry points; nothing that was there changes.)  The
   arguments, t_out, a0_out[i * 2 + g], the checks, the T < 2^27 refusal and the chunk protocol are those of
   scape_hip_report_boot_len and scape_hip_report_boot_usage, except that n_groups must be 2: any other value is refused.
   With A_g, Q_g, a_ig of those two entry points the device forms, in those entry points' kernel bodies with both
   populations in one series (every nonzero still read once, or twice for a usage record of more than 8 kept rows),
     d(b)   = (double)Q_0(b) / (double)A_0(b) - (double)Q_1(b) / (double)A_1(b)          (boot_len_diff)
     d_i(b) = (double)a_i0(b) / (double)A_0(b) - (double)a_i1(b) / (double)A_1(b)        (boot_usage_diff)
   two IEEE divisions and one IEEE subtraction, contraction off: bit for bit v_0(b) - v_1(b) and u_i0(b) - u_i1(b) of the
   entry points above;  +infinity when A_0(b) = 0 or A_1(b) = 0.  A value is never -0.0 (x - x = +0.0 under round to
   nearest, and the quotients are never -0).  d(b) is stored at column b - 1 of vals[r][n_boot], d_i(b) of vals[k][n_boot],
   k = the index of the kept row in `rows`, in the array of boot_len; the record set belongs to the entry point that
   began it, and a later chunk through any other of the four is refused.  No LDS, no atomics: both populations' sums live
   in registers. */
int scape_hip_report_boot_len_diff(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                   int32_t n_groups, const int32_t *seg_off, const int32_t *q, int64_t n_boot,
                                   int64_t *t_out, int64_t *a0_out);
int scape_hip_report_boot_usage_diff(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                     int32_t n_groups, const int32_t *seg_off, int64_t n_boot, int64_t *t_out,
                                     int64_t *a0_out);
/* The n_boot values of one series of the last record set, whichever of the four entry points wrote it: boot_len (record
   r, group g: series = r * n_groups + g), boot_usage (kept row k, group g: series = k * n_groups + g), boot_len_diff
   (series = r) or boot_usage_diff (series = k). */
int scape_hip_report_boot_vals_get(scape_hip_ctx *ctx, int64_t series, double *vals_out);
/* Per series of the last record set of those four, over its n_boot values and a level of level_bp basis points
   (1 .. 9999):
     n_def_out = D = #{b in 1..n_boot : the value is defined},   k = max(1, floor((D + 1) * (10000 - level_bp) / 20000)) in integers,
     lo_out = the k-th smallest value,   hi_out = the (D + 1 - k)-th smallest;   both +infinity when D = 0
   by a radix select (no sort, no cap on n_boot) over key(x) = bits(x) ^ (bits(x) >> 63 ? ~0 : 1 << 63), which is
   monotone over the finite doubles of either sign and puts +infinity above them all; a value is defined when key <
   key(+infinity), and the result is the inverse map of the selected key.  Over non-negative values the keys order as
   the bit patterns do.  Refused unless every column 1 .. n_boot has been written since the array was allocated. */
int scape_hip_report_boot_quantiles(scape_hip_ctx *ctx, int32_t level_bp, double *lo_out, double *hi_out,
                                    int64_t *n_def_out);
/* wait for a slot's text; *host_ptr stays valid until the next render into that slot or scape_hip_report_free */
int scape_hip_report_fetch(scape_hip_ctx *ctx, int32_t slot, void **host_ptr, int64_t *bytes_out);
/* per record, the cluster codes present (id2code == NULL: every read in code 0) -> n_groups_out[r]; then
   scape_hip_report_hist_fetch returns the codes (ascending per record, records in order) and the counts
   [group][K[r] + 1] per record (slot K = reads with label >= K).  Nothing is queued when bad_read_out reports a read. */
int scape_hip_report_hist(scape_hip_ctx *ctx, int32_t n_rec, const int64_t *read_off, const int32_t *K,
                          const int64_t *label, const int64_t *cb_id, int64_t id_min, int64_t id_span,
                          const int32_t *id2code, int32_t n_codes, int64_t *n_groups_out, int64_t *bad_read_out);
int scape_hip_report_hist_fetch(scape_hip_ctx *ctx, int64_t n_groups, int32_t *codes_out, int64_t n_hist,
                                int32_t *hist_out);
/* release every buffer of the reporting stages (also done by scape_hip_destroy) */
int scape_hip_report_free(scape_hip_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
