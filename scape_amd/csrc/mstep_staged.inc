// mstep_staged.inc - k2_mstep: the M-step with both MFMA operands staged global -> VGPR -> LDS.
// (included by scape_hip.hip after mstep.inc, whose frame it shares with k3_mstep and k4_mstep: identical bits.  Runs
// under SCAPE_HIP_MSTEP=v2 and when the job vectors exceed the 32-bit offsets of the LDS-DMA kernels.)
//
// One workgroup per (UTR, MT_ROWS-row tile).  D[rows x jobs] = Mtile[rows x n] * V[n x jobs] on the f64
// matrix cores (v_mfma_f64_16x16x4_f64): wave w owns MT_RB blocks of 16 rows, job columns come in groups
// of 16.  Operand maps (cdna_hip_programming.md section 3): A lane l = A[row l&15][k l>>4],
// B lane l = B[k l>>4][col l&15], D lane l reg i = D[row (l>>4)+4i][col l&15].
// Both operands are staged through LDS as they lie in memory ([row][n] and [job][n], pitch 34 f64: one
// 16-byte store per loaded double2, fragment reads free of bank conflicts); the global loads of chunks
// c+1 and c+2 are in flight during the MFMAs of chunk c (two register stages).  The kernel is a stream over
// the tensor: every tile is read once per round, so HBM bandwidth bounds it, not the MFMA rate.

#define MT_NC 32                      // bins per chunk
#define MT_PITCH (MT_NC + 2)          // LDS pitch (f64) of the [row][n] image: rows 272 B apart -> 16-B aligned double2
#define MT_VPITCH (MT_NC + 2)         // stores, and (2*row + k) mod 32 distinct within every 32-lane read group
                                      // (ds_read_b64 banking, MI355X_MICROARCH.md section LDS): conflict-free fragments
#ifndef MT_DV1
#define MT_DV1 1      // the job vectors (L2-resident) are requested one chunk ahead, the tensor tile two: frees 4 G registers (-3 % launch time)
#endif
#ifndef MT_DEEP
#define MT_DEEP 2                     // register stages of the M-step's loads in passes of <= 32 jobs (measured: 3 and 4 change nothing, big calls or small)
#endif

// G = 16-job column groups of the pass, D = chunks of global loads in flight per wavefront (register stages):
// passes with few jobs have the registers for a deeper pipeline, and they are the ones that wait on memory
// rather than on the matrix cores
template <int G, int D>
__device__ __forceinline__ void mstep_pass(const double *__restrict__ Mu, const double *__restrict__ V,
                                           const int64_t *__restrict__ voff, const int *s_jobs, double *mt,
                                           double *vt, int cnt, int Np, int n_lo, int n_hi, int nrows, int row0, int wave, int lane,
                                           int need, v4f64 (&acc)[MT_RB][MT_MAXJ / 16]) {
    const int quarter = lane >> 4, ns = 2 * (lane & 15);   // staging: 4 rows (or jobs) x 32 n per wave-instruction
    const int kq = lane >> 4, rc = lane & 15;              // fragments
    constexpr int DV = MT_DV1 ? 1 : D;                // chunks of job-vector loads in flight (they come from L2)
    double2 rm_st[D][4 * MT_RB], rv_st[DV][G];              // D chunks of global loads in flight
    const double *vsrc[G];
#pragma unroll
    for (int it = 0; it < G; ++it) {
        const int js = 4 * wave + quarter + 16 * it;
        vsrc[it] = (js < cnt) ? V + voff[s_jobs[js]] : nullptr;
    }
    auto fetchV = [&](int n0, double2 (&rv)[G]) {
        const int nc = (n_hi - n0 < MT_NC) ? n_hi - n0 : MT_NC;
#pragma unroll
        for (int it = 0; it < G; ++it)
            rv[it] = (ns < nc && vsrc[it]) ? *reinterpret_cast<const double2 *>(vsrc[it] + n0 + ns) : make_double2(0.0, 0.0);
    };
    auto fetchM = [&](int n0, double2 (&rm)[4 * MT_RB]) {
        const int nc = (n_hi - n0 < MT_NC) ? n_hi - n0 : MT_NC;   // <= 0 past the end: nothing is loaded
#pragma unroll
        for (int it = 0; it < 4 * MT_RB; ++it) {
            const int row = row0 + 4 * wave + quarter + 16 * it;
            // iteration `it` stages the 16-row group that MFMA wave it/MT_RB consumes; groups outside every
            // job's window are not read (their scores are never looked at)
            rm[it] = (ns < nc && row < nrows && ((need >> (it / MT_RB)) & 1)) ? *reinterpret_cast<const double2 *>(Mu + (size_t)row * Np + n0 + ns)
                                               : make_double2(0.0, 0.0);
        }
    };
    auto chunk = [&](int n0, double2 (&rm)[4 * MT_RB], double2 (&rv)[G]) {
        const int nc = (n_hi - n0 < MT_NC) ? n_hi - n0 : MT_NC;  // multiple of 16
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 4 * MT_RB; ++it) {
            const int rr = 4 * wave + quarter + 16 * it;
            *reinterpret_cast<double2 *>(&mt[rr * MT_PITCH + ns]) = rm[it];
        }
#pragma unroll
        for (int it = 0; it < G; ++it) {
            const int js = 4 * wave + quarter + 16 * it;
            *reinterpret_cast<double2 *>(&vt[js * MT_VPITCH + ns]) = rv[it];
        }
        __syncthreads();
        fetchM(n0 + D * MT_NC, rm);
        fetchV(n0 + DV * MT_NC, rv);
        // one k-step per trip: 1 + G fragment reads, then G MFMAs (the compiler does not unroll this).  Measured and
        // not kept: the reads of k-step i+1 issued before the MFMAs of k-step i (2.24 -> 2.38 ms per launch), two
        // k-steps per trip (2.19 -> 2.33 ms) - longer MFMA bursts per wavefront interleave worse with the two
        // neighbours on the SIMD and the two barriers per chunk; s_setprio raised around the MFMA loop, or around the
        // staging part instead (no change).
#pragma unroll 4
        for (int n4 = 0; n4 < nc; n4 += 4) {
            double a[MT_RB], b[G];
#pragma unroll
            for (int rb = 0; rb < MT_RB; ++rb) a[rb] = mt[(16 * (MT_RB * wave + rb) + rc) * MT_PITCH + n4 + kq];
#pragma unroll
            for (int g = 0; g < G; ++g) b[g] = vt[(16 * g + rc) * MT_VPITCH + n4 + kq];
#pragma unroll
            for (int rb = 0; rb < MT_RB; ++rb)
#pragma unroll
                for (int g = 0; g < G; ++g)
                    acc[rb][g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rb], b[g], acc[rb][g], 0, 0, 0);
        }
    };
#pragma unroll
    for (int dd = 0; dd < D; ++dd) fetchM(n_lo + dd * MT_NC, rm_st[dd]);
#pragma unroll
    for (int dd = 0; dd < DV; ++dd) fetchV(n_lo + dd * MT_NC, rv_st[dd]);
    for (int n0 = n_lo; n0 < n_hi; n0 += D * MT_NC) {
#pragma unroll
        for (int dd = 0; dd < D; ++dd)
            if (n0 + dd * MT_NC < n_hi) chunk(n0 + dd * MT_NC, rm_st[dd], rv_st[dd % DV]);
    }
}

__global__ __launch_bounds__(256, 3) void k2_mstep(MSTEP_PARAMS(tiles_max), int jobs_per_pass, unsigned long long *__restrict__ dbg) {
    __shared__ __attribute__((aligned(16))) double mt[MT_ROWS * MT_PITCH];   // [row][n]
    __shared__ __attribute__((aligned(16))) double vt[MT_MAXJ * MT_VPITCH];  // [job slot][n]
    __shared__ int s_jobs[MT_MAXJ];
    __shared__ int s_all[1024];               // jobs of this UTR whose window covers the tile
    __shared__ int s_cnt, s_nlo, s_nhi, s_need, s_first;
    __shared__ double s_ps[4][MT_MAXJ];
    __shared__ int s_pr[4][MT_MAXJ];
    __shared__ double s_tail[MT_MAXJ];          // per job: sum of v over the bins beyond the tile's finite extent
    __shared__ int s_wcnt[4];
    __shared__ unsigned long long s_by[3];
    int ul, t;
    if (!mstep_block(blockIdx.x, n_utr, tiles_max, ul, t)) return;
    const int u = active[ul];   // only UTRs that have jobs in this call get workgroups
    const UtrDesc d = descs[u];
    const int B = P.B, Np = d.Np;
    const int nrows = d.T * B, row0 = t * MT_ROWS;
    if (row0 >= nrows) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *Mu = M + (size_t)d.m_off;
    const int found = mstep_collect(ujob_list, ujob_off[u], ujob_off[u + 1], rd_m, rd_lo, rd_hi, row0, tid, lane, wave, s_wcnt, [&](int off, int j) {
        if (off < 1024) s_all[off] = j;
    });
    if (tid == 0) s_cnt = found;
    __syncthreads();
    const int total = min(s_cnt, 1024);
    if (dbg && tid == 0) mstep_debug_tile(dbg, total);
    if (total == 0) return;
    if (tid == 0) s_by[0] = s_by[1] = s_by[2] = 0ull;

    // a tile with more than MT_MAXJ jobs needs several passes; with gridDim.y > 1 (small calls, where a workgroup's
    // serial time is what counts) the passes of a tile are taken by different workgroups
    // jobs_per_pass (16 / 32 / 64, a call-wide constant): calls with few live tiles, where a round takes as long as
    // ONE workgroup's pass over its tile, cut the job list into short passes that gridDim.y workgroups take in
    // parallel - every score is the same MFMA chain whichever workgroup and column group computes it
    for (int base = (int)blockIdx.y * jobs_per_pass; base < total; base += jobs_per_pass * (int)gridDim.y) {
        const int cnt = min(jobs_per_pass, total - base);
        const int G = (cnt + 15) >> 4;
        __syncthreads();
        if (wave == 0) {   // cnt <= 64: one job per lane of the first wavefront, reductions by shuffles (no LDS atomics)
            MstepWin w;
            if (lane < cnt) {
                const int j = s_all[base + lane];
                s_jobs[lane] = j;
                w = mstep_window_of_job(rd_lo[j], rd_hi[j], rd_n0[j], rd_n1[j], row0, t);
            }
            w = mstep_window_reduce(w);
            if (lane == 0) {
                s_need = w.mk;
                s_nlo = w.nlo;
                s_nhi = w.nhi;
                s_first = w.first;
            }
        }
        __syncthreads();
        const int n_ext = tile_nend[d.tile_off + t];
        const MstepSpan sp = mstep_span(s_nlo, s_nhi, Np, n_ext);
        const int need = s_need;
        if (tid == 0 && sp.nh > 0) mstep_tally(s_by, need, nrows, row0, sp.nh, cnt, s_first);
        for (int sj = tid; sj < cnt; sj += 256) {
            const int j = s_jobs[sj];
            s_tail[sj] = Vsuf[mstep_tail_index(voff[j], j, n_ext)];
        }
        __syncthreads();
        v4f64 acc[MT_RB][MT_MAXJ / 16];
#pragma unroll
        for (int rb = 0; rb < MT_RB; ++rb)
#pragma unroll
            for (int g = 0; g < MT_MAXJ / 16; ++g) acc[rb][g] = (v4f64){0.0, 0.0, 0.0, 0.0};
        switch (G) {
            case 1: mstep_pass<1, MT_DEEP>(Mu, V, voff, s_jobs, mt, vt, cnt, Np, sp.n_lo, sp.n_hi, nrows, row0, wave, lane, need, acc); break;
            case 2: mstep_pass<2, MT_DEEP>(Mu, V, voff, s_jobs, mt, vt, cnt, Np, sp.n_lo, sp.n_hi, nrows, row0, wave, lane, need, acc); break;
            case 3: mstep_pass<3, 2>(Mu, V, voff, s_jobs, mt, vt, cnt, Np, sp.n_lo, sp.n_hi, nrows, row0, wave, lane, need, acc); break;
            default: mstep_pass<4, 2>(Mu, V, voff, s_jobs, mt, vt, cnt, Np, sp.n_lo, sp.n_hi, nrows, row0, wave, lane, need, acc); break;
        }
        // per job: arg-max over this wave's 16 rows, then over the 4 waves
        const int kq = lane >> 4, rc = lane & 15;
#pragma unroll
        for (int g = 0; g < MT_MAXJ / 16; ++g) {
            if (g < G) {
                const int slot_j = 16 * g + rc;
                MstepBest b;
                if (slot_j < cnt) {
                    const int j = s_jobs[slot_j];
                    const int lo = rd_lo[j], hi = rd_hi[j];
                    const double c0 = mstep_c0(rd_lw[j], rd_sv[j], s_tail[slot_j]);
#pragma unroll
                    for (int rb = 0; rb < MT_RB; ++rb)
                        b = mstep_best_of_rows(b, acc[rb][g], c0, lo, hi, row0 + 16 * (MT_RB * wave + rb) + kq, nrows);
                }
                b = mstep_merge_lanes(b);
                if (kq == 0 && slot_j < cnt) {
                    s_ps[wave][slot_j] = b.score;
                    s_pr[wave][slot_j] = b.row;
                }
            }
        }
        __syncthreads();
        for (int sj = tid; sj < cnt; sj += 256) {
            const MstepBest b = mstep_merge_waves(&s_ps[0][0], &s_pr[0][0], MT_MAXJ, sj);
            const int j = s_jobs[sj];
            pt_score[ptoff[j] + t] = b.score;
            pt_row[ptoff[j] + t] = mstep_row_or_fallback(b.row, rd_lo[j], row0);
        }
    }
    if (tid == 0) mstep_tally_flush(counters, s_by);
}
