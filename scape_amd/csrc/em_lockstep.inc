// em_lockstep.inc - the batched EM of scape_hip.hip: all jobs advance in lock-step rounds.
// (included by scape_hip.hip; uses its UtrDesc / DevParams / d_* helpers)
//
// Why: the 100 (K, restart) jobs of a UTR all scan the SAME marginal tensor in their grid arg-max
// M-step (apa_core.py:507-523).  Job-at-a-time kernels re-read the tensor once per job and round
// (30 GB per UTR at the headline shape for a 35 MB tensor).  Here every round is two launches:
//   k2_estep  one wavefront per job: finish the previous M-step (reduce per-tile partial arg-maxes),
//             refresh the stale column, responsibilities / weight update / ELBO / stopping rule,
//             and publish v = Z[:,k]*cnt plus the (row window, log w_k) of this round's M-step;
//   an M-step one workgroup per (UTR, 64-row tile of the [T*B, N] tensor): the tile is multiplied on the f64 matrix
//             cores with the v vectors of EVERY job of that UTR whose window covers it; the per-(job, tile) arg-max
//             goes to a partial table that the next k2_estep reduces in row order (first-maximum tie rule).
//             (mstep.inc: the frame; mstep_staged.inc, mstep_ring.inc, mstep_multi.inc: k2_mstep, k3_mstep, k4_mstep.)
// This file is the E-step and the shrink kernel, and the constants that they, the M-step and the host share.

#define MT_RB 1                      // 16-row blocks per wave
#define MT_ROWS (64 * MT_RB)          // tensor rows per tile: 4 waves x MT_RB x 16
#define MT_MAXJ 64                    // jobs (columns) of one M-step pass over a tile
// Run-ahead: between two M-step launches (one PASS over the tensor) a job executes up to EM_DEPTH consecutive rounds, as
// long as the next round's component is neither equal nor adjacent to one whose grid arg-max is still pending (see
// k2_estep), and publishes one M-step column (v vector, window, log w_k) per round.  Everything the M-step reads or
// writes is per COLUMN, column id = job * depth + slot; depth is the call's runtime cap <= EM_DEPTH (SCAPE_HIP_EM_DEPTH).
#ifndef EM_DEPTH
#define EM_DEPTH 3
#endif
static_assert(EM_DEPTH >= 1 && EM_DEPTH <= 8, "column slots per job");
// device counters (unsigned long long each): [0] rounds, [1] unused, [2] z elements, [3] finalised jobs, then
// 64-way sharded: slab elements, executed job-rounds, and the M-step's own byte tallies
#define CNT_DONE 3                    // jobs finalised in this call (one add per job lifetime; read with the early-exit probe)
#define CNT_SLAB 4
#define CNT_EXEC (4 + 64)
#define CNT_MSTEP_TENSOR (4 + 2 * 64)
#define CNT_MSTEP_VREQ (4 + 3 * 64)
#define CNT_MSTEP_VUNI (4 + 4 * 64)
static_assert(MT_ROWS == TILE_ROWS, "tile height must match k_tile_extent / the host tables");
static_assert(MT_MAXJ <= 64, "the per-pass job setup gives one job to each lane of one wavefront");

struct EmState {
    int32_t *ia, *ib, *sia, *sib;     // [n_jobs*kmax] current / snapshot grid indices
    double *ws, *slw;                 // [n_jobs*(kmax+1)] weights / snapshot log-weights
    double *lb, *ell;                 // [n_jobs]
    int32_t *nlb, *status;            // [n_jobs]   rounds executed; status: 0 running, 1 stop after pending M-step, 2 done
    unsigned long long *pend;         // [n_jobs]   run-ahead state of the current pass: bit c + 1 = component c has a column published
                                      //            in it, bit 0 = the job runs its next round in the pass's next E-step launch
    // per column (= job * depth + slot; [n_jobs * depth]) from here on
    int32_t *rd_k, *rd_lo, *rd_hi, *rd_m;   // round descriptor: component, row window [lo,hi), has M-step
    int32_t *rd_n0, *rd_n1;           // bins [n0,n1) outside which v is exactly 0
    double *rd_lw, *rd_sv;            // log w_k (new), sum_n v[n]
    double *rd_fl;                    // the score of a row that is all sentinel on the support of v: log w_k sum v + SENT sum v
    double *V;                        // ragged [column][Np]
    double *Vsuf;                     // ragged [column][Np/16 + 1]: Vsuf[b] = sum_{n >= 16 b} V[n] (summed from the end)
    const int64_t *voff;              // [columns]
    double *pt_score;                 // ragged [column][n_tiles(utr)]
    int32_t *pt_row;
    const int64_t *ptoff;             // [columns]
    int32_t *u_done;                  // [n_utr] finalised jobs of each UTR in this call (em_rounds' shrink); null: not counted
};

__device__ __forceinline__ double d_wave_allsum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;  // identical in every lane
}

// Build switches of the throughput E-step (must precede estep_body: its `#if ESTEP_EXP_GROUP` is read where it stands).
// ESTEP_EXP_GROUP: exp chains of neighbouring components interleaved in groups of this size; 1 = one at a time.  Measured at the
// end of round 3 on one box, E-step ms per sweep: 1 -> 36.9-37.4 (the default: it is what every earlier build of this round ran,
// the switch used to be defined BELOW its first use and read as 0 there), 2 -> 36.7-36.8, 4 at two wavefronts per SIMD
// (-DESTEP_WPS=2) -> 36.3-36.4, 6 at two -> 36.1-36.9: the kernel is insensitive to how its latency is hidden.
#ifndef ESTEP_EXP_GROUP
#define ESTEP_EXP_GROUP 1
#endif
// f(integral_constant<c>) for the component c == k of a register array of CMAX, k wave-uniform and held in a scalar
// register: one scalar branch tree per use.  Written as `if (c == k)` inside the unrolled component loop the same thing
// is two v_cndmask_b32 per f64 and component for every value the branch assigns (10 per component and bin for the
// sumk / rescue / zk group of the bin step); a dynamic index z[k] would move the array out of registers.
template <int CMAX, class F>
__device__ __forceinline__ void d_at_uniform(int k, F &&f) {
#define AT_CASE(i)                                                 \
    case i:                                                        \
        if constexpr ((i) < CMAX) f(std::integral_constant<int, (i)>{}); \
        break;
#define AT_CASE8(b) AT_CASE(b) AT_CASE(b + 1) AT_CASE(b + 2) AT_CASE(b + 3) AT_CASE(b + 4) AT_CASE(b + 5) AT_CASE(b + 6) AT_CASE(b + 7)
    switch (k) {
        AT_CASE8(0) AT_CASE8(8) AT_CASE8(16) AT_CASE8(24) AT_CASE8(32) AT_CASE8(40) AT_CASE8(48) AT_CASE8(56)
        default: break;
    }
#undef AT_CASE8
#undef AT_CASE
}
// The row entropy's accumulation en += -pk * d without its guard `(pk > 0) ? ... : 0.0`, rounded as the guarded form was
// compiled: the first component (en is the literal +0.0 there) one fma onto +0.0, every later one the product rounded
// on its own, then the sum.  pk >= 0 and d is finite, so with pk == 0 the term is +-0, and +-0 added to an accumulator
// that started at +0.0 changes nothing; likewise `ell` without its `z != 0` guard (one fma, as it was compiled).
__device__ __forceinline__ double d_en_add(bool first, double en, double pk, double d) {
#pragma clang fp contract(off)
    if (first) return __builtin_fma(-pk, d, 0.0);
    const double t = -pk * d;
    return en + t;
}
// A shift by N lanes towards lane 0 inside each row of 16 lanes (DPP row_shl, two 32-bit halves; lanes whose source
// lies beyond the row read +0.0) - in-register, where __shfl_down goes through the LDS crossbar.
template <int N>
__device__ __forceinline__ double d_row_shl(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x100 + N, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x100 + N, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double d_lane_value(double v, int l) {      // v of lane l, wave-uniform (two v_readlane_b32)
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// Body of one E-step for one job.  CA = compile-time array/loop bound; CX = the job's exact column count
// K+1 when the caller dispatched on it (every `c < C` test then folds away), 0 = runtime C <= CA.
// NW = wavefronts that work on the job: 1 (k2_estep: the throughput kernel) or 4 (k2_estep_cs, calls with few jobs):
// the four wavefronts walk the SAME bins in the same order and split the COMPONENTS of a bin - exps, weight sums and
// their lane reductions of component c belong to wavefront c mod 4, the row sums are recomputed by every wavefront
// from the exchanged values, the ELBO / entropy chains stay on wavefront 0.  Every sum keeps the operand order of the
// one-wavefront kernel, so both return identical bits.
struct EstepNext {      // what one call of estep_body tells its kernel about the job (wave-uniform)
    int status;         // the job's status now: 0 running, 1 stop after the pending M-step, 2 finalised
    int nlb;            // rounds the job has executed
    int pub_k;          // component whose M-step column this round published, -1: none
    int k_next;         // component of round nlb (meaningful while nlb < nround)
};

template <int CA, int CX, int NW = 1>
__device__ __forceinline__ EstepNext estep_body(
    const UtrDesc *__restrict__ descs, const DevParams &P, const double *__restrict__ cnt,
    const double *__restrict__ M, int kmax, const int32_t *__restrict__ job_utr,
    const int32_t *__restrict__ job_K, const int32_t *__restrict__ job_fixed,
    const int32_t *__restrict__ a_in, const int32_t *__restrict__ b_in,
    const double *__restrict__ ws_in, const int8_t *__restrict__ k_arr, const EmState &S,
    int32_t *__restrict__ a_out, int32_t *__restrict__ b_out, double *__restrict__ ws_out,
    double *__restrict__ bic_out, int32_t *__restrict__ nlb_out, double *__restrict__ lb_out,
    unsigned long long *__restrict__ counters, int launch, int slot, int depth, int job, int lane, int status,
    unsigned long long *s_roff, double *s_lwc, double *s_wsum /* [CA][64] per-lane weight numerators */,
    const double2 *s_exptab /* d_load_exptab */, int wave = 0, double *s_xz = nullptr /* [2][CA][64] */,
    double *s_tot = nullptr /* [CA + 4] */) {
    constexpr int CMAX = CA;
#ifdef ESTEP_STAMPS
    const unsigned long long st0 = __builtin_amdgcn_s_memtime();
#define ESTEP_STAMP(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#else
#define ESTEP_STAMP(v)
#endif
    const bool lead = (NW == 1) || wave == 0;     // the wavefront that runs the serial parts of the round
    const int nround = P.nround, B = P.B;
    // ---- set-up.  Everything whose address depends on `job` alone is requested HERE, in one batch; what depends on
    // those values (the UTR descriptor, the per-tile partial arg-maxes) in a second one.  (Written as the reference
    // reads - value by value, each behind the branch that needs it - the set-up was 7-8 dependent round trips to L2,
    // 15 % of a job-round's lifetime.)  Per-column state sits in lane c and is handed around by shuffles.
    const int u_job = job_utr[job];
    // (K, the round counter, the round's component and the grid indices derived from it are wave-uniform; taken through
    // readfirstlane they live in scalar registers, and every test on them is a scalar branch, not a per-lane select)
    const int K = (CX > 0) ? CX - 1 : __builtin_amdgcn_readfirstlane(job_K[job]), C = K + 1;
    const bool fixed = job_fixed[job] != 0;
    int32_t *ia = S.ia + (size_t)job * kmax, *ib = S.ib + (size_t)job * kmax;
    int32_t *sia = S.sia + (size_t)job * kmax, *sib = S.sib + (size_t)job * kmax;
    double *ws = S.ws + (size_t)job * (kmax + 1), *slw = S.slw + (size_t)job * (kmax + 1);
    // The job's round is its own counter S.nlb, not the launch index.  Call `slot` of pass `launch` publishes into column
    // col0 + slot; the first call of a pass (slot 0) finishes the grid arg-maxes of every column the previous pass
    // published - their components are pairwise neither equal nor adjacent (k2_estep), so the order is immaterial;
    // slot order = round order.
    const bool r0 = launch == 0 && slot == 0;
    const bool resolve = slot == 0 && launch > 0;
    const size_t col0 = (size_t)job * depth, col = col0 + slot;
    int pre_m[EM_DEPTH], pre_lo[EM_DEPTH], pre_hi[EM_DEPTH], pre_k[EM_DEPTH];
    int64_t pre_ptoff[EM_DEPTH];
    double pre_fl[EM_DEPTH];
    bool rdm = false;
#pragma unroll
    for (int q = 0; q < EM_DEPTH; ++q) {
        const bool on = resolve && q < depth;
        pre_m[q] = on ? S.rd_m[col0 + q] : 0;
        pre_lo[q] = on ? S.rd_lo[col0 + q] : 0;
        pre_hi[q] = on ? S.rd_hi[col0 + q] : 0;
        pre_k[q] = on ? S.rd_k[col0 + q] : 0;
        pre_ptoff[q] = on ? S.ptoff[col0 + q] : 0;
        pre_fl[q] = on ? S.rd_fl[col0 + q] : 0.0;
        rdm = rdm || pre_m[q] != 0;
    }
    const int64_t pre_voff = S.voff[col];
    // the job's component order sits in lanes 0 .. nround - 1 (one request with the rest of this batch; indexed by the
    // round counter it would be one more dependent trip)
    const int k_lane = (lane < nround) ? (int)k_arr[(size_t)job * nround + lane] : 0;
    const double lb_prev = r0 ? SENT : S.lb[job];       // (read after the bin loop these two were one more trip at the end)
    const int nlb_prev = r0 ? 0 : __builtin_amdgcn_readfirstlane(S.nlb[job]);
    auto k_of_round = [&](int i) {
        const int ii = min(i, nround - 1);
        return (nround <= 64) ? __shfl(k_lane, ii, 64) : (int)k_arr[(size_t)job * nround + ii];
    };
    const int k_now = __builtin_amdgcn_readfirstlane(k_of_round(nlb_prev));
    const int k_next = __builtin_amdgcn_readfirstlane(k_of_round(nlb_prev + 1));
    double my_ws = 0.0, my_slw = 0.0;                    // lane c < C: weight / snapshot log-weight of column c
    int my_ia = 0, my_ib = 0, my_sia = 0, my_sib = 0;    // lane c < K: current / snapshot grid indices
    if (lane < C) {
        my_ws = r0 ? ws_in[(size_t)job * (kmax + 1) + lane] : ws[lane];
        if (!r0) my_slw = slw[lane];
        if (lane < K) {
            my_ia = r0 ? a_in[(size_t)job * kmax + lane] : ia[lane];
            my_ib = r0 ? b_in[(size_t)job * kmax + lane] : ib[lane];
            my_sia = r0 ? my_ia : sia[lane];
            my_sib = r0 ? my_ib : sib[lane];
        }
    }
    // second batch
    const UtrDesc d = descs[u_job];
    double pt_best[EM_DEPTH];
    int pt_best_r[EM_DEPTH];
#pragma unroll
    for (int q = 0; q < EM_DEPTH; ++q) {
        pt_best[q] = -INFINITY;
        pt_best_r[q] = pre_lo[q];
        if (pre_m[q]) {   // per-tile partials of a pending grid arg-max (wave-uniform condition)
            const int t0 = pre_lo[q] / MT_ROWS, t1 = (pre_hi[q] - 1) / MT_ROWS;
            // Rows that are all sentinel on the support of v are tied exactly (max_alpha_beta gives the first of them),
            // but a tile sums the sentinel terms below its finite extent by the MFMA chain and the rest from the suffix
            // sums: tiles of different extent round the same score differently, and a later tile could win.  Every such
            // evaluation lies within (4 Np + 16) u of the floor (Np roundings each for the suffix sums and the chain, on
            // either side): a tile score that close to the floor IS the floor, and the first tile keeps the tie.  A row with
            // a finite entry that cannot lift it out of that band cannot be told from the floor by any f64 evaluation.
            const double fl = pre_fl[q], ftol = (4.0 * d.Np + 16.0) * 1.1102230246251565e-16 * fabs(fl);
            for (int t = t0 + lane; t <= t1; t += 64) {
                double sc = S.pt_score[pre_ptoff[q] + t];
                const int rr = S.pt_row[pre_ptoff[q] + t];
                if (fabs(sc - fl) <= ftol) sc = fl;
                if (sc > pt_best[q]) {
                    pt_best[q] = sc;
                    pt_best_r[q] = rr;
                }
            }
        }
    }
    const int N = d.N, Np = d.Np;
    const double *Mu = M + (size_t)d.m_off;
    const double *cu = cnt + d.bin_off;
    if (r0) my_slw = d_logw(my_ws);

    if (lead && r0) {  // em_algo prologue (:715-724)
        if (lane < C) {
            ws[lane] = my_ws;
            slw[lane] = my_slw;
            if (lane < K) {
                ia[lane] = sia[lane] = my_ia;
                ib[lane] = sib[lane] = my_ib;
            }
        }
        if (lane == 0) {
            S.lb[job] = SENT;
            S.nlb[job] = 0;
            S.ell[job] = 0.0;
        }
    }
    int upd_k[EM_DEPTH], upd_a[EM_DEPTH], upd_b[EM_DEPTH];   // alpha/beta indices just decided (not yet re-read from memory)
#pragma unroll
    for (int q = 0; q < EM_DEPTH; ++q) {
        upd_k[q] = -1;
        upd_a[q] = upd_b[q] = 0;
        if (pre_m[q]) {
            // finish max_alpha_beta of a published round: first maximum over the tiles, in row order
            double best = pt_best[q];
            int best_r = pt_best_r[q];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ob = __shfl_xor(best, off, 64);
                const int orr = __shfl_xor(best_r, off, 64);
                if (ob > best || (ob == best && orr < best_r)) {
                    best = ob;
                    best_r = orr;
                }
            }
            upd_k[q] = pre_k[q];
            upd_a[q] = best_r / B;
            upd_b[q] = best_r - upd_a[q] * B;
            if (lead && lane == 0) {
                ia[upd_k[q]] = upd_a[q];
                ib[upd_k[q]] = upd_b[q];
            }
            if (lane == upd_k[q]) {      // lane c keeps column c's current indices
                my_ia = upd_a[q];
                my_ib = upd_b[q];
            }
        }
    }
    // every slot of the job is free again (slot 0 only: later calls of a pass keep what the earlier ones published)
    if (slot == 0 && lead && lane == 0 && (r0 || rdm))
        for (int q = 0; q < depth; ++q) S.rd_m[col0 + q] = 0;
    auto cur_ia = [&](int i) {     // (memory forms: the once-per-job finalisation on lane 0)
        int v = ia[i];
#pragma unroll
        for (int q = 0; q < EM_DEPTH; ++q) v = (i == upd_k[q]) ? upd_a[q] : v;
        return v;
    };
    auto cur_ib = [&](int i) {
        int v = ib[i];
#pragma unroll
        for (int q = 0; q < EM_DEPTH; ++q) v = (i == upd_k[q]) ? upd_b[q] : v;
        return v;
    };

    if (status == 1 || nlb_prev >= nround) {
        // cal_bic (:702-706), sort by alpha (:768-772), outputs
        if (lead && lane == 0) {
            const int n_lb = S.nlb[job];
            bic_out[job] = d_bic(S.ell[job], K, N);
            nlb_out[job] = n_lb;
            int idx[CMAX];
            for (int i = 0; i < K; ++i) idx[i] = i;
            for (int i = 1; i < K; ++i) {
                const int v = idx[i];
                int j = i - 1;
                while (j >= 0 && cur_ia(idx[j]) > cur_ia(v)) {
                    idx[j + 1] = idx[j];
                    --j;
                }
                idx[j + 1] = v;
            }
            for (int i = 0; i < K; ++i) {
                a_out[(size_t)job * kmax + i] = cur_ia(idx[i]);
                b_out[(size_t)job * kmax + i] = cur_ib(idx[i]);
                ws_out[(size_t)job * (kmax + 1) + i] = ws[idx[i]];
            }
            ws_out[(size_t)job * (kmax + 1) + K] = ws[K];
            for (int i = K; i < kmax; ++i) {
                a_out[(size_t)job * kmax + i] = -1;
                b_out[(size_t)job * kmax + i] = -1;
                ws_out[(size_t)job * (kmax + 1) + i + 1] = 0.0;
            }
            S.status[job] = 2;
            atomicAdd(&counters[CNT_DONE], 1ull);
            if (S.u_done) atomicAdd(&S.u_done[u_job], 1);
            atomicAdd(&counters[0], (unsigned long long)n_lb);
            atomicAdd(&counters[2], (unsigned long long)n_lb * (unsigned long long)N * (unsigned long long)C);
        }
        return EstepNext{2, nlb_prev, -1, 0};
    }

    // ---- round nlb_prev of em_algo (:726-746) --------------------------------------------------
    // executed job-rounds (host early-exit probe); the two per-job-round counters are kept in 64 shards each
    // (counters[4..67] slab elements, counters[68..131] executed) - one address would take 51,200 adds per launch
    if (lead && lane == 0) atomicAdd(&counters[CNT_EXEC + (job & 63)], 1ull);
    const int k = k_now;
    // cal_z_k(para, k) (:731): refresh the snapshot of column k (every lane computes it, lane 0 stores it)
    const double wk_old = __shfl(my_ws, k, 64);
    const double slw_k = d_logw(wk_old);
    const int sia_k = (k < K) ? __builtin_amdgcn_readlane(my_ia, k) : 0;
    const int sib_k = (k < K) ? __builtin_amdgcn_readlane(my_ib, k) : 0;
    // neighbours of component k in the UNSORTED current alpha list: the M-step window of this round (:511-514)
    const int ia_km1 = __builtin_amdgcn_readlane(my_ia, max(k - 1, 0)), ia_kp1 = __builtin_amdgcn_readlane(my_ia, min(k + 1, 63));
    if (lead && lane == 0) {
        slw[k] = slw_k;
        if (k < K) {
            sia[k] = sia_k;
            sib[k] = sib_k;
        }
    }
    // column descriptors (tensor row offset, snapshot log-weight) live in LDS, not in registers:
    // the kernel is latency-bound, so what matters is how many wavefronts fit on a SIMD
    if (lead && lane < CMAX) {
        const int c = lane;
        int sa = 0, sb = 0;
        double lw_c = 0.0;
        if (c < C) {
            if (c == k) {
                lw_c = slw_k;
                sa = sia_k;
                sb = sib_k;
            } else {
                lw_c = my_slw;
                sa = my_sia;
                sb = my_sib;
            }
        }
        s_roff[c] = (c < K) ? ((unsigned long long)sa * B + sb) * Np : 0ull;
        s_lwc[c] = (c < K) ? lw_c : lw_c + d.unif_ll;      // uniform column: the whole log-Z value
    }
    __syncthreads();
    double *Vj = S.V + pre_voff;

    ESTEP_STAMP(st1);
    double tot_w[CMAX], t_sumk = 0.0, t_ell = 0.0, t_ent = 0.0;
    int nz_lo = 0x7fffffff, nz_hi = -1;   // first / last bin of this lane with v != 0
    const ExpPoly exp_poly = d_exp_poly_held();       // (scape_hip.hip: no copy in front of a Horner step)
    const LogPoly log_poly = d_log_poly_held();
    // One pass over the bins; mod = the pass adds the rescue 1e-8 to column k.  The first pass never does and the second
    // always does, so `mod` is a compile-time constant of the pass: the first pass (all but a handful of job-rounds run
    // no other) carries no select, branch or log for the rescue.  Returns: the pass must be redone with the rescue.
    if constexpr (NW == 1) {
        auto run_pass = [&](auto mod_c) {
            constexpr bool mod = decltype(mod_c)::value;
    #pragma unroll
            for (int c = 0; c < CMAX; ++c) s_wsum[c * 64 + lane] = 0.0;
            double sumk = 0.0, ell = 0.0, ent = 0.0;
            nz_lo = 0x7fffffff;
            nz_hi = -1;
            auto fetch = [&](int n, double (&m)[CMAX], double &cn) {
                const bool ok = n < N;
                cn = ok ? cu[n] : 0.0;
    #pragma unroll
                for (int c = 0; c < CMAX; ++c) m[c] = (ok && c < K) ? Mu[s_roff[c] + n] : 0.0;
            };
            // one bin of this lane, n < Np, from its tensor values mcur and read count ccur
            auto bin_step = [&](int n, const double (&mcur)[CMAX], double ccur) {
                double vkn = 0.0;
                if (n < N) {
                    const double cn = ccur;
                    // log Z value of column c (recomputed where needed: one LDS read + add is cheaper than a
                    // 12-entry register array at this kernel's occupancy)
                    auto lzv = [&](int c) { return (c < K) ? s_lwc[c] + mcur[c] : s_lwc[c]; };
                    double mx = 0.0;
    #pragma unroll
                    for (int c = 0; c < CMAX; ++c) {
                        if (c < C) {
                            const double v = lzv(c);
                            mx = (c == 0) ? v : fmax(mx, v);       // (v_max_f64: the values are finite, never NaN)
                        }
                    }
                    // exp underflows to exactly 0 below -745.14; when that holds for the whole wavefront the
                    // component is skipped (bins are sorted by position, so lanes agree most of the time)
                    double z[CMAX];
                    unsigned long long live = 0ull;
#if ESTEP_EXP_GROUP >= 2
                    // components in groups of ESTEP_EXP_GROUP (neighbours in alpha, so their liveness goes together): the
                    // exp chains of a group - each with a table read in the middle - are independent and interleave; exp of
                    // an argument below -746 is exactly 0, the value a skipped component gets, so the bits are those of the
                    // one-at-a-time loop
    #pragma unroll
                    for (int c = 0; c < CMAX; c += ESTEP_EXP_GROUP) {
    #pragma unroll
                        for (int i = 0; i < ESTEP_EXP_GROUP; ++i)
                            if (c + i < CMAX) z[c + i] = 0.0;
                        if (c < C) {
                            double arg[ESTEP_EXP_GROUP];
                            bool any_live = false;
    #pragma unroll
                            for (int i = 0; i < ESTEP_EXP_GROUP; ++i) {
                                const bool in = (c + i < CMAX) && (c + i < C);
                                arg[i] = in ? (lzv((c + i < CMAX) ? c + i : c) - mx) * cn : -1000.0;
                                any_live |= arg[i] >= -746.0;
                            }
                            if (__ballot(any_live)) {
    #pragma unroll
                                for (int i = 0; i < ESTEP_EXP_GROUP; ++i)
                                    if (c + i < CMAX)
                                        if (c + i < C) {
                                            live |= 1ull << (c + i);
                                            z[c + i] = d_exp_nonpos(arg[i], s_exptab, exp_poly);
                                        }
                            }
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
#else
    #pragma unroll
                    for (int c = 0; c < CMAX; ++c) {
                        z[c] = 0.0;
                        if (c < C) {
                            const double arg = (lzv(c) - mx) * cn;
                            if (__ballot(arg >= -746.0)) {
                                live |= 1ull << c;
                                z[c] = d_exp_nonpos(arg, s_exptab, exp_poly);
                            }
                            // keep the scheduler from interleaving all CMAX exp chains (it would spend ~100
                            // extra VGPRs on that; occupancy hides the latency instead)
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
#endif
                    const double s = d_np_sum<CMAX>(z, C);
                    const double rs = d_rcp_mid(s);   // one reciprocal per bin (1 <= s <= K+1): z * (1/s) is within 2 ulp of z / s (norm_z :494)
                    double zk = 0.0;
    #pragma unroll
                    for (int c = 0; c < CMAX; ++c) z[c] = z[c] * rs;     // a skipped component is +0.0 and stays +0.0 (0 < rs <= 1)
                    d_at_uniform<CMAX>(k, [&](auto ck) {
                        constexpr int c = decltype(ck)::value;
                        zk = z[c];
                        if (mod) z[c] += 1e-8;
                    });
                    sumk += zk;                // Z[:,k] before the rescue
                    if (mod) zk += 1e-8;       // (the same sum as z[k] just took)
                    // entropy of the row (scipy.stats.entropy re-normalises by s2): log pk_c is known in
                    // closed form, log z_c = (lz_c - mx)*cn - log s, so only two logs per bin are needed
                    const double s2 = d_np_sum<CMAX>(z, C);
                    // s2 = sum of the normalised row = 1 +- a few ulp (1 + 1e-8 when the rescue fired): log(s2) by its
                    // series, exact to f64 for |s2 - 1| < 1e-4 (next term x^3/3 < 4e-13 * |x|... < 1 ulp of x)
                    const double x2 = s2 - 1.0;
                    const double ls = d_log_pos(s, log_poly), rs2 = d_rcp_mid(s2);   // s >= 1: the row maximum contributes exp(0); s2 = 1 +- tiny
                    double ls2 = x2 - 0.5 * x2 * x2;
                    if (__ballot(fabs(x2) >= 1e-5)) ls2 = (fabs(x2) < 1e-5) ? ls2 : log(s2);   // wave-uniform: normally skipped
                    double lzk_mod = 0.0;
                    if constexpr (mod) lzk_mod = log(zk);   // one log, not one per unrolled component
                    double en = 0.0;
    #pragma unroll
                    for (int c = 0; c < CMAX; ++c) {
                        if (c < C && ((live & (1ull << c)) || (mod && c == k))) {
                            const double lzc_full = lzv(c);
                            s_wsum[c * 64 + lane] = __builtin_fma(cn, z[c], s_wsum[c * 64 + lane]);
                            ell = __builtin_fma(z[c] * cn, lzc_full, ell);           // (no `z != 0` / `pk > 0` guards: see d_en_add)
                            const double pk = z[c] * rs2;      // s2 = 1 +- few ulp: z/s2 and z*(1/s2) agree to 1 ulp
                            const double lzc = (mod && c == k) ? lzk_mod : (lzc_full - mx) * cn - ls;
                            en = d_en_add(c == 0, en, pk, lzc - ls2);
                        }
                    }
                    ent += cn * en;
                    vkn = zk * cn;
                }
                Vj[n] = vkn;
                if (vkn != 0.0) {
                    nz_lo = min(nz_lo, n);
                    nz_hi = n;
                }
            };
            // software pipeline over the bins of this lane: the tensor values of the next bin are requested before the
            // current bin's exp/div chain runs.  (One bin per trip and the hand-over copy `mcur = mnext`, a v_mov_b64 per
            // column and bin: two bins per trip with the two buffers swapping roles has no copy but twice the loop's code,
            // and measured 1 % slower - profiles/estep_bin_step.txt.)
            double mcur[CMAX], mnext[CMAX], ccur = 0.0, cnext = 0.0;
            fetch(lane, mcur, ccur);
            // the first bin's values must have ARRIVED before the loop: otherwise the compiler's wait-count pass sees loads
            // pending on mcur at the loop header and puts vmcnt(1) / vmcnt(0) in front of their first use in EVERY iteration -
            // right behind the requests for the next bin, which are then waited for at once (the counter is in issue order)
    #pragma unroll
            for (int c = 0; c < CMAX; ++c) asm volatile("" : "+v"(mcur[c]));
            asm volatile("" : "+v"(ccur));
            for (int n = lane; n < Np; n += 64) {
                fetch(n + 64, mnext, cnext);
                bin_step(n, mcur, ccur);
    #pragma unroll
                for (int c = 0; c < CMAX; ++c) mcur[c] = mnext[c];
                ccur = cnext;
            }
    #pragma unroll
            for (int c = 0; c < CMAX; ++c) tot_w[c] = d_wave_allsum(s_wsum[c * 64 + lane]);
            t_sumk = d_wave_allsum(sumk);
            t_ell = d_wave_allsum(ell);
            t_ent = d_wave_allsum(ent);
            return !mod && t_sumk < 1e-8;
        };
        if (run_pass(std::false_type{})) run_pass(std::true_type{});   // Z[:,k] += 1e-8 (apa_core.py:528-529): redo the pass
    } else {
        // ---- NW wavefronts, components split (see the comment above estep_body) ---------------------------------
        auto run_pass = [&](auto mod_c) {
            constexpr bool mod = decltype(mod_c)::value;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if ((c % NW) == wave) s_wsum[c * 64 + lane] = 0.0;
            double sumk = 0.0, ell = 0.0, ent = 0.0;
            nz_lo = 0x7fffffff;
            nz_hi = -1;
            double mcur[CMAX], ccur = 0.0;
            auto fetch = [&](int n, double (&m)[CMAX], double &cn) {
                const bool ok = n < N;
                cn = ok ? cu[n] : 0.0;
#pragma unroll
                for (int c = 0; c < CMAX; ++c) m[c] = (ok && c < K) ? Mu[s_roff[c] + n] : 0.0;
            };
            fetch(lane, mcur, ccur);
#pragma unroll
            for (int c = 0; c < CMAX; ++c) asm volatile("" : "+v"(mcur[c]));    // arrived before the loop (see the one-wavefront path)
            asm volatile("" : "+v"(ccur));
            int buf = 0;
            // the trip count must be the same for every lane and wavefront (barrier and ballots inside): the loop runs
            // on the wave-uniform n0, lanes past the row (Np is a multiple of 16, not of 64) are predicated off
            for (int n0 = 0; n0 < Np; n0 += 64, buf ^= 1) {
                const int n = n0 + lane;
                double mnext[CMAX], cnext;
                fetch(n + 64, mnext, cnext);
                double *xz = s_xz + (size_t)buf * (CMAX * 64);
                const double cn = ccur;
                auto lzv = [&](int c) { return (c < K) ? s_lwc[c] + mcur[c] : s_lwc[c]; };
                double mx = 0.0;
                if (n < N) {
#pragma unroll
                    for (int c = 0; c < CMAX; ++c) {
                        if (c < C) {
                            const double v = lzv(c);
                            mx = (c == 0) ? v : fmax(mx, v);       // (v_max_f64: the values are finite, never NaN)
                        }
                    }
                    // this wavefront's components: the un-normalised responsibilities go to the exchange buffer
#pragma unroll
                    for (int c = 0; c < CMAX; ++c) {
                        if (c < C && (c % NW) == wave) {
                            const double arg = (lzv(c) - mx) * cn;
                            double zr = 0.0;
                            if (__ballot(arg >= -746.0)) zr = d_exp_nonpos(arg, s_exptab, exp_poly);
                            xz[c * 64 + lane] = zr;
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                }
                __syncthreads();       // one barrier per step: the buffers alternate
                double vkn = 0.0;
                if (n < N) {
                    double z[CMAX];
#pragma unroll
                    for (int c = 0; c < CMAX; ++c) z[c] = (c < C) ? xz[c * 64 + lane] : 0.0;
                    const double s = d_np_sum<CMAX>(z, C);
                    const double rs = d_rcp_mid(s);
                    double zk = 0.0;
#pragma unroll
                    for (int c = 0; c < CMAX; ++c) z[c] = z[c] * rs;
                    d_at_uniform<CMAX>(k, [&](auto ck) {
                        constexpr int c = decltype(ck)::value;
                        zk = z[c];
                        if (mod) z[c] += 1e-8;
                    });
                    sumk += zk;                // Z[:,k] before the rescue
                    if (mod) zk += 1e-8;       // (the same sum as z[k] just took)
                    const double s2 = d_np_sum<CMAX>(z, C);
                    const double x2 = s2 - 1.0;
                    const double ls = d_log_pos(s, log_poly), rs2 = d_rcp_mid(s2);
                    double ls2 = x2 - 0.5 * x2 * x2;
                    if (__ballot(fabs(x2) >= 1e-5)) ls2 = (fabs(x2) < 1e-5) ? ls2 : log(s2);
                    double lzk_mod = 0.0;
                    if constexpr (mod) lzk_mod = log(zk);
#pragma unroll
                    for (int c = 0; c < CMAX; ++c)
                        if (c < C && (c % NW) == wave) s_wsum[c * 64 + lane] = __builtin_fma(cn, z[c], s_wsum[c * 64 + lane]);
                    if (lead) {
                        double en = 0.0;
#pragma unroll
                        for (int c = 0; c < CMAX; ++c) {
                            if (c < C) {
                                const double lzc_full = lzv(c);
                                ell = __builtin_fma(z[c] * cn, lzc_full, ell);
                                const double pk = z[c] * rs2;
                                const double lzc = (mod && c == k) ? lzk_mod : (lzc_full - mx) * cn - ls;
                                en = d_en_add(c == 0, en, pk, lzc - ls2);
                            }
                        }
                        ent += cn * en;
                        vkn = zk * cn;
                    }
                }
                if (lead && n < Np) {
                    Vj[n] = vkn;
                    if (vkn != 0.0) {
                        nz_lo = min(nz_lo, n);
                        nz_hi = n;
                    }
                }
#pragma unroll
                for (int c = 0; c < CMAX; ++c) mcur[c] = mnext[c];
                ccur = cnext;
            }
            // lane reductions by the owning wavefronts, totals to wavefront 0 through LDS
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                if ((c % NW) == wave) {
                    const double t = d_wave_allsum(s_wsum[c * 64 + lane]);
                    if (lane == 0) s_tot[c] = t;
                }
            }
            if (lead) {
                t_sumk = d_wave_allsum(sumk);
                t_ell = d_wave_allsum(ell);
                t_ent = d_wave_allsum(ent);
                if (lane == 0) s_tot[CMAX] = (!mod && t_sumk < 1e-8) ? 1.0 : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < CMAX; ++c) tot_w[c] = s_tot[c];
            const bool redo = s_tot[CMAX] != 0.0;
            __syncthreads();           // s_tot and the exchange buffers are rewritten by a second pass
            return redo;
        };
        if (run_pass(std::false_type{})) run_pass(std::true_type{});   // Z[:,k] += 1e-8 (apa_core.py:528-529): redo the pass
        if (!lead) return EstepNext{0, 0, -1, 0};
    }

    ESTEP_STAMP(st2);
    // maximize_ws (:498-505)
    double sv = 0.0;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
        if (c == k) sv = tot_w[c];
    double wn[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) wn[c] = (c < C) ? tot_w[c] : 0.0;
    {
        const double s = d_np_sum<CMAX>(wn, C);
#pragma unroll
        for (int c = 0; c < CMAX; ++c) wn[c] = wn[c] / s;
        double wK = 0.0;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c == K) wK = wn[c];
        if (wK > P.max_unif_ws) {
            const double sk = d_np_sum<CMAX>(wn, K);
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                if (c < K) wn[c] = (1 - P.max_unif_ws) * wn[c] / sk;
                if (c == K) wn[c] = P.max_unif_ws;
            }
        }
    }
    double wk_new = 0.0;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        if (c == k) wk_new = wn[c];
        if (c == lane && c < C) ws[c] = wn[c];
    }

#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nz_lo = min(nz_lo, __shfl_xor(nz_lo, off, 64));
        nz_hi = max(nz_hi, __shfl_xor(nz_hi, off, 64));
    }
    ESTEP_STAMP(st3);
    double v_total = 0.0;             // sum_n v[n] as the suffix sums have it (Vsuf[0])
    if (!fixed && k < K) {
        // suffix sums of v at 16-bin boundaries, accumulated from the last bin backwards (a tail of 1e-100
        // next to a head of 1e3 must come out as 1e-100: the M-step multiplies it by the sentinel)
        double *Sj = S.Vsuf + (pre_voff >> 4) + col;
        double carry = 0.0;
        // v is read back in batches of 8 groups of 64 bins (one round trip to L2 per batch instead of one per group:
        // the 17-34 dependent trips of a group-at-a-time loop were a quarter of a wavefront's lifetime); the sums
        // themselves run group by group from the last one, in the same order as before
        for (int nb = ((Np - 1) >> 6) << 6; nb >= 0; nb -= 8 * 64) {
            double vv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int n = nb - 64 * q + lane;
                vv[q] = (n >= 0 && n < Np) ? Vj[n] : 0.0;
            }
            // Of a Hillis-Steele scan over the 64 lanes of a group (steps 1, 2, .. 32, each lane adding the lane `step`
            // above it) only the sums S(0), S(16), S(32), S(48) that start at a 16-bin boundary are used.  Steps 1, 2, 4, 8
            // leave in the first lane of row r (16 lanes) the row's sum T_r in the order of a balanced tree and never
            // reach across a row from there: they are row-local DPP shifts, in registers.  Steps 16 and 32 then give
            // S(48) = T3, S(32) = T2 + T3, S(16) = (T1 + T2) + T3, S(0) = (T0 + T1) + (T2 + T3) - formed here from the four
            // row heads as wave-uniform values, bit for bit what the six trips through the LDS crossbar returned
            // (tools/estep_scan_check.cpp).  The eight groups of a batch are independent of one another (only the carry
            // links them); groups below bin 0 scan zeros and are not stored.
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                vv[q] += d_row_shl<1>(vv[q]);
                vv[q] += d_row_shl<2>(vv[q]);
                vv[q] += d_row_shl<4>(vv[q]);
                vv[q] += d_row_shl<8>(vv[q]);
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int n0 = nb - 64 * q;
                if (n0 >= 0) {                        // wave-uniform
                    const int n = n0 + lane;
                    const double T0 = d_lane_value(vv[q], 0), T1 = d_lane_value(vv[q], 16), T2 = d_lane_value(vv[q], 32),
                                 T3 = d_lane_value(vv[q], 48);
                    const double S32 = T2 + T3, S16 = (T1 + T2) + T3, S0 = (T0 + T1) + S32;
                    const double mine = (lane < 16) ? S0 : (lane < 32) ? S16 : (lane < 48) ? S32 : T3;
                    if ((lane & 15) == 0 && n < Np) Sj[n >> 4] = carry + mine;
                    carry += S0;
                }
            }
        }
        if (lane == 0) Sj[Np >> 4] = 0.0;
        v_total = carry;
    }
    ESTEP_STAMP(st4);
    // elbo (:559-561), stopping rule (:743-746), this round's M-step descriptor (:507-523)
    const double lb_new = t_ell + t_ent;                 // (the wavefront sums are identical in every lane)
    const int status_new = (fabs(lb_new - lb_prev) < fabs(1e-6 * lb_prev)) ? 1 : 0;
    const bool has_m = (!fixed && k < K);
    if (lane == 0) {
        const int n_lb = nlb_prev;
        lb_out[(size_t)job * nround + n_lb] = lb_new;
        S.nlb[job] = n_lb + 1;
        S.ell[job] = t_ell;
        S.lb[job] = lb_new;
        S.status[job] = status_new;
        S.rd_m[col] = has_m ? 1 : 0;
        if (has_m) {
            const int lo = (k == 0) ? 0 : ia_km1;
            const int hi = (k == K - 1) ? d.T - 1 : ia_kp1;
            S.rd_k[col] = k;
            S.rd_lo[col] = lo * B;
            S.rd_hi[col] = (hi + 1) * B;
            S.rd_lw[col] = d_logw(wk_new);
            S.rd_sv[col] = sv;
            S.rd_fl[col] = d_logw(wk_new) * sv + SENT * v_total;
            S.rd_n0[col] = (nz_hi >= 0) ? nz_lo : 0;
            S.rd_n1[col] = (nz_hi >= 0) ? nz_hi + 1 : 0;
            atomicAdd(&counters[CNT_SLAB + (job & 63)], (unsigned long long)(hi + 1 - lo) * B * (unsigned long long)N);
        }
    }
#ifdef ESTEP_STAMPS
    if (NW == 1 && lane == 0) {
        const unsigned long long st5 = __builtin_amdgcn_s_memtime();
        unsigned long long *sp = counters + 4 + 5 * 64;
        atomicAdd(&sp[0], st1 - st0);
        atomicAdd(&sp[1], st2 - st1);
        atomicAdd(&sp[2], st3 - st2);
        atomicAdd(&sp[3], st4 - st3);
        atomicAdd(&sp[4], st5 - st4);
        atomicAdd(&sp[7], 1ull);
    }
#endif
#undef ESTEP_STAMP
    return EstepNext{status_new, nlb_prev + 1, has_m ? k : -1, k_next};
}

// one code variant per exact column count K+1 <= 16 (every `c < C` test folds away), selected per job - a
// wave-uniform branch; kernels built for more columns (CM = 24, 32) run the generic body with runtime predication
// (ROUND = launch index; `slot`, `depth` and the result `nx` are variables of the calling scope)
#define ESTEP_ARGS(ROUND, STATUS) descs, P, cnt, M, kmax, job_utr, job_K, job_fixed, a_in, b_in, ws_in, k_arr, S, a_out, \
                   b_out, ws_out, bic_out, nlb_out, lb_out, counters, ROUND, slot, depth, job, lane, STATUS, s_roff, s_lwc, s_wsum, s_exptab
#define ESTEP_CASE(C, ROUND, STATUS) \
    case C: nx = estep_body<C, C, ESTEP_NW>(ESTEP_ARGS(ROUND, STATUS) ESTEP_EXTRA); break;
#define ESTEP_DISPATCH(CM, ROUND, STATUS)                                                         \
    do {                                                                                          \
        if constexpr (CM <= 16) {                                                                 \
            const int c_exact = job_K[job] + 1;                                                   \
            if constexpr (CM >= 16) {                                                             \
                if (c_exact > 12) {                                                               \
                    switch (c_exact) {                                                            \
                        ESTEP_CASE(13, ROUND, STATUS) ESTEP_CASE(14, ROUND, STATUS)               \
                        ESTEP_CASE(15, ROUND, STATUS)                                             \
                        default: nx = estep_body<16, 16, ESTEP_NW>(ESTEP_ARGS(ROUND, STATUS) ESTEP_EXTRA); break;            \
                    }                                                                             \
                    break;                                                                        \
                }                                                                                 \
            }                                                                                     \
            if constexpr (CM >= 12) {                                                             \
                if (c_exact > 8) {                                                                \
                    switch (c_exact) {                                                            \
                        ESTEP_CASE(9, ROUND, STATUS) ESTEP_CASE(10, ROUND, STATUS)                \
                        ESTEP_CASE(11, ROUND, STATUS)                                             \
                        default: nx = estep_body<12, 12, ESTEP_NW>(ESTEP_ARGS(ROUND, STATUS) ESTEP_EXTRA); break;            \
                    }                                                                             \
                    break;                                                                        \
                }                                                                                 \
            }                                                                                     \
            if constexpr (CM >= 8) {                                                              \
                if (c_exact > 4) {                                                                \
                    switch (c_exact) {                                                            \
                        ESTEP_CASE(5, ROUND, STATUS) ESTEP_CASE(6, ROUND, STATUS)                 \
                        ESTEP_CASE(7, ROUND, STATUS)                                              \
                        default: nx = estep_body<8, 8, ESTEP_NW>(ESTEP_ARGS(ROUND, STATUS) ESTEP_EXTRA); break;              \
                    }                                                                             \
                    break;                                                                        \
                }                                                                                 \
            }                                                                                     \
            switch (c_exact) {                                                                    \
                ESTEP_CASE(1, ROUND, STATUS) ESTEP_CASE(2, ROUND, STATUS) ESTEP_CASE(3, ROUND, STATUS) \
                default: nx = estep_body<4, 4, ESTEP_NW>(ESTEP_ARGS(ROUND, STATUS) ESTEP_EXTRA); break;                      \
            }                                                                                     \
        } else {                                                                                  \
            nx = estep_body<CM, 0, ESTEP_NW>(ESTEP_ARGS(ROUND, STATUS) ESTEP_EXTRA);                                       \
        }                                                                                         \
    } while (0)

// The schedule rule of the run-ahead (host and device; tools/em_schedule_check.cpp restates and checks it): after a round
// that left the job at `status` with `nlb` rounds executed, does the pass stop in front of round nlb, whose component
// is k_next?  pend: bit c + 1 set = component c has a column published in this pass.  (The slot count is the host's:
// it launches `depth` slots per pass.)
__host__ __device__ inline bool em_run_ahead_stops(int status, int nlb, int nround, int k_next, unsigned long long pend) {
    return status != 0 || nlb >= nround || (pend & (7ull << k_next)) != 0ull;
}
// The slots a pass can use at all, from the largest K among the live ordinary jobs (0: only fixed-inference jobs are
// live, which run one round per pass): the columns of a pass belong to components that are pairwise neither equal nor
// adjacent, so K <= 2 never runs ahead and K = 3 only over the pair (0, 2).  Holds for component orders over 0 .. K - 1
// (gen_k_arr); a round of the uniform component K publishes nothing and could run ahead further - with a slot missing
// the job runs that round in the next pass, same bits.  em_rounds launches this many k2_estep slots after a shrink.
__host__ inline int em_slots_needed(int max_k_live, int depth) {
    return std::min(depth, max_k_live <= 2 ? 1 : max_k_live == 3 ? 2 : depth);
}
// Is a list of `listed` entries, `live` of them still needed, due for compaction at threshold `pct` (percent)?
__host__ inline bool em_shrink_due(long long listed, long long live, int pct) {
    return live > 0 && live < listed && live * 100 <= listed * pct;
}
// Stable compaction, one chunk of the list per step and one entry per thread: where the entry of lane `lane` of wavefront
// `wave` goes, given the entries kept before this chunk (base), the kept counts of the chunk's wavefronts and the
// wavefront's own keep mask.  (k_em_shrink; tools/em_schedule_check.cpp replays it on the host.)
__host__ __device__ inline int em_shrink_pos(int base, const int *wave_cnt, int wave, unsigned long long mask, int lane) {
    int off = base;
    for (int w = 0; w < wave; ++w) off += wave_cnt[w];
    unsigned long long below = mask & ((1ull << lane) - 1ull);
    int n = 0;
    for (; below; below &= below - 1) ++n;
    return off + n;
}

// The shrink of a call that runs ahead (em_rounds): one workgroup rewrites, in place and in order,
//   elist  without the jobs at status 2 (a job at status 1 still has its finalising E-step to run and stays), and
//   active without the UTRs all of whose jobs are finalised (u_done[u] = the UTR's job count),
// and writes out[0] = jobs kept, out[1] = UTRs kept, out[2] = largest K among the kept ordinary jobs (0: none).
// In place is safe: a chunk is read whole before any of it is written, and it writes at or below where it read.
#define EM_SHRINK_THREADS 1024
#ifndef EM_SHRINK_AT
#define EM_SHRINK_AT 50               // default of SCAPE_HIP_EM_SHRINK_AT (percent of a list still live; profiles/em_shrink.txt)
#endif
__global__ __launch_bounds__(EM_SHRINK_THREADS) void k_em_shrink(int32_t *elist, int n_list, const int32_t *__restrict__ status,
                                                                 const int32_t *__restrict__ job_K, const int32_t *__restrict__ job_fixed,
                                                                 int32_t *active, int n_active, const int32_t *__restrict__ u_done,
                                                                 const int64_t *__restrict__ ujob_off, int depth, int32_t *__restrict__ out) {
    __shared__ int s_cnt[EM_SHRINK_THREADS / 64];
    __shared__ int s_k;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_k = 0;
    int k_live = 0;
    auto compact = [&](int32_t *list, int n, auto keep) {
        int base = 0;
        for (int i0 = 0; i0 < n; i0 += EM_SHRINK_THREADS) {
            const int i = i0 + tid;
            int32_t v = 0;
            bool kp = false;
            if (i < n) {
                v = list[i];
                kp = keep(v);
            }
            const unsigned long long mask = __ballot(kp);
            if (lane == 0) s_cnt[wave] = __popcll(mask);
            __syncthreads();
            if (kp) list[em_shrink_pos(base, s_cnt, wave, mask, lane)] = v;
            for (int w = 0; w < EM_SHRINK_THREADS / 64; ++w) base += s_cnt[w];
            __syncthreads();
        }
        return base;
    };
    const int jobs = compact(elist, n_list, [&](int32_t j) {
        const bool live = status[j] != 2;
        if (live && job_fixed[j] == 0) k_live = max(k_live, job_K[j]);
        return live;
    });
    const int utrs = compact(active, n_active, [&](int32_t u) { return (int64_t)u_done[u] * depth < ujob_off[u + 1] - ujob_off[u]; });
    if (k_live) atomicMax(&s_k, k_live);
    __syncthreads();
    if (tid == 0) {
        out[0] = jobs;
        out[1] = utrs;
        out[2] = s_k;
    }
}
#define ESTEP_NW 1
#ifndef ESTEP_WPS
#define ESTEP_WPS 3      // wavefronts per SIMD the throughput E-step is compiled for (4 was measured: see DESIGN.md)
#endif
#define ESTEP_EXTRA
// more than 12 columns: 2 wavefronts per SIMD (up to 256 registers) instead of 3 with the column arrays spilled
template <int CMAX>
__global__ __launch_bounds__(64, (CMAX > 12 ? 2 : ESTEP_WPS)) void k2_estep(
    const UtrDesc *__restrict__ descs, DevParams P, const double *__restrict__ cnt,
    const double *__restrict__ M, int kmax, const int32_t *__restrict__ job_utr,
    const int32_t *__restrict__ job_K, const int32_t *__restrict__ job_fixed,
    const int32_t *__restrict__ a_in, const int32_t *__restrict__ b_in,
    const double *__restrict__ ws_in, const int8_t *__restrict__ k_arr, EmState S,
    int32_t *__restrict__ a_out, int32_t *__restrict__ b_out, double *__restrict__ ws_out,
    double *__restrict__ bic_out, int32_t *__restrict__ nlb_out, double *__restrict__ lb_out,
    unsigned long long *__restrict__ counters, int launch, int slot, int depth, const int32_t *__restrict__ job_list,
    int n_jobs) {
    // jobs are ordered UTR-major; blocks b and b+8 share an XCD, so give each XCD a contiguous job range:
    // the jobs of one UTR (which re-read the same few tensor rows) then meet in one L2.  Speed only.
    const int chunk = (n_jobs + 7) >> 3;
    const int jidx = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
    if (jidx >= n_jobs) return;
    const int job = job_list[jidx];
    const int lane = threadIdx.x;
    const int status = (launch == 0 && slot == 0) ? 0 : S.status[job];
    if (status == 2) return;
    // Run-ahead.  A pass is `depth` launches of this kernel (slot 0, 1, ...) and one M-step launch.  A round reads the
    // alpha / beta of its own component c (column refresh, apa_core.py:731) and the alpha of c - 1 and c + 1 (its M-step
    // window, :511-514) and nothing else of the grid arg-max, so a job goes on to its next round in the same pass unless
    // that round's component is equal or adjacent to one whose arg-max is pending, i.e. published earlier in the pass.  It
    // also stops after the round that meets the stopping rule and after round nround - 1.  A round's arithmetic is
    // estep_body's whichever slot it runs in, so the job's bits do not depend on depth.  (One launch per slot and not a
    // loop over the slots in here: with the loop the compiler keeps 25-35 more VGPRs live across the bin loop - what
    // k2_estep_all_rounds shows against this kernel - and the 12-column variants spill inside it; a wavefront that has
    // nothing to do in a slot leaves right here.)
    unsigned long long pend = 0ull;
    if (slot > 0) {
        pend = S.pend[job];
        if (!(pend & 1ull)) return;
        pend &= ~1ull;
    }
    // column descriptors (tensor row offset, snapshot log-weight) and the per-lane weight numerators live in
    // LDS, not in registers: what matters here is how many wavefronts fit on a SIMD
    __shared__ unsigned long long s_roff[CMAX];
    __shared__ double s_lwc[CMAX];
    __shared__ double s_wsum[CMAX * 64];
    __shared__ double2 s_exptab[128];
    d_load_exptab(s_exptab, lane, 64);
    EstepNext nx;
    ESTEP_DISPATCH(CMAX, launch, status);
    if (depth > 1 && lane == 0) {
        if (nx.pub_k >= 0) pend |= 2ull << nx.pub_k;
        // fixed-inference jobs have no M-step, nothing to share a tensor pass for: one round per pass, as before
        const bool stop = em_run_ahead_stops(nx.status, nx.nlb, P.nround, nx.k_next, pend) || job_fixed[job] != 0;
        S.pend[job] = pend | (stop ? 0ull : 1ull);
    }
}

// Jobs that never need an M-step (fixed inference, the ws-only re-fit of rm_component, apa_core.py:708-711) have
// no cross-workgroup dependency between rounds: one launch runs all their rounds, one wavefront per job.
// Lane 0's state writes of round r must be visible to every lane in round r+1: agent-scope fence between rounds
// (store release + L1 invalidate); the per-round kernels get the same effect from the launch boundary.
template <int CMAX>
__global__ __launch_bounds__(64, (CMAX > 12 ? 2 : 3)) void k2_estep_all_rounds(
    const UtrDesc *__restrict__ descs, DevParams P, const double *__restrict__ cnt,
    const double *__restrict__ M, int kmax, const int32_t *__restrict__ job_utr,
    const int32_t *__restrict__ job_K, const int32_t *__restrict__ job_fixed,
    const int32_t *__restrict__ a_in, const int32_t *__restrict__ b_in,
    const double *__restrict__ ws_in, const int8_t *__restrict__ k_arr, EmState S,
    int32_t *__restrict__ a_out, int32_t *__restrict__ b_out, double *__restrict__ ws_out,
    double *__restrict__ bic_out, int32_t *__restrict__ nlb_out, double *__restrict__ lb_out,
    unsigned long long *__restrict__ counters, const int32_t *__restrict__ job_list, int n_jobs) {
    const int chunk = (n_jobs + 7) >> 3;
    const int jidx = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
    if (jidx >= n_jobs) return;
    const int job = job_list[jidx];
    const int lane = threadIdx.x;
    __shared__ unsigned long long s_roff[CMAX];
    __shared__ double s_lwc[CMAX];
    __shared__ double s_wsum[CMAX * 64];
    __shared__ double2 s_exptab[128];
    d_load_exptab(s_exptab, lane, 64);
    for (int round = 0; round <= P.nround; ++round) {     // (a call of fixed-inference jobs has one column slot per job)
        const int status = (round == 0) ? 0 : S.status[job];
        if (status == 2) return;
        constexpr int slot = 0, depth = 1;
        EstepNext nx;
        ESTEP_DISPATCH(CMAX, round, status);
        (void)nx;
        __threadfence();
        __syncthreads();
    }
}
#undef ESTEP_NW
#undef ESTEP_EXTRA
#define ESTEP_NW 4
#define ESTEP_EXTRA , wave, s_xz, s_tot
// The same round for calls with few jobs (the reference-stream modes: the ~100 jobs of ONE UTR per call), where a
// round takes as long as one wavefront needs for its 17 dependent bin steps: one workgroup of 4 wavefronts per job,
// the components of a bin split over them (estep_body, NW = 4).  Identical bits to k2_estep.
template <int CMAX>
__global__ __launch_bounds__(256, 1) void k2_estep_cs(
    const UtrDesc *__restrict__ descs, DevParams P, const double *__restrict__ cnt,
    const double *__restrict__ M, int kmax, const int32_t *__restrict__ job_utr,
    const int32_t *__restrict__ job_K, const int32_t *__restrict__ job_fixed,
    const int32_t *__restrict__ a_in, const int32_t *__restrict__ b_in,
    const double *__restrict__ ws_in, const int8_t *__restrict__ k_arr, EmState S,
    int32_t *__restrict__ a_out, int32_t *__restrict__ b_out, double *__restrict__ ws_out,
    double *__restrict__ bic_out, int32_t *__restrict__ nlb_out, double *__restrict__ lb_out,
    unsigned long long *__restrict__ counters, int round, const int32_t *__restrict__ job_list, int n_jobs) {
    const int chunk = (n_jobs + 7) >> 3;
    const int jidx = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
    if (jidx >= n_jobs) return;
    const int job = job_list[jidx];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int status = (round == 0) ? 0 : S.status[job];
    if (status == 2) return;
    __shared__ unsigned long long s_roff[CMAX];
    __shared__ double s_lwc[CMAX];
    __shared__ double s_wsum[CMAX * 64];
    __shared__ double s_xz[2 * CMAX * 64];
    __shared__ double s_tot[CMAX + 4];
    __shared__ double2 s_exptab[128];
    d_load_exptab(s_exptab, threadIdx.x, 256);
    constexpr int slot = 0, depth = 1;   // one round per launch, one column slot per job (the host runs small calls at depth 1)
    EstepNext nx;
    ESTEP_DISPATCH(CMAX, round, status);
    (void)nx;
}
#undef ESTEP_NW
#undef ESTEP_EXTRA
#undef ESTEP_DISPATCH
#undef ESTEP_CASE
