// phase_b.inc - Phase B of the tensor build (included by scape_hip.hip behind Phase A; needs d_exp_nonpos, d_log_pos,
// d_logpdf_normal, SENT, TILE_ROWS and UtrDesc).
// Reference: get_loglik_marginal_tensor / loglik_marginal_lxr, taichi_core.py:160-246:
//   M[i][j][n] = logsumexp_w( A[n,w] + log N(theta_w; theta_i, beta_j) - G_ij ) over the +-3 beta window (:218-234).
// r-unknown bins take the linear-domain form log( sum_w V[w][n] * exp(g_w - G) ) - mathematically the same sum, no exp
// per term - on the f64 matrix cores; bins whose A was built in the log domain (pA-site / r-known) take the reference's
// two-pass form.  Three forms give the same bits (the host's choice: phase_b_choose); what differs is who computes what,
// and how often:
//   form 0  k_phase_b: one workgroup per (UTR, alpha = theta_i) does everything.  It stays for non-uniform theta grids,
//           for more than 16 beta values and for the operator seam (every bin in the log domain).
//   form 1  k_pb_tables + k_phase_b_lin (B <= 16).  The windows, the normaliser and the weight tile ran on 13 threads at
//           the head of every 256-thread workgroup of form 0 (1.9 of its 15 ms), the log-domain bins' 2 x W dependent
//           load -> exp steps at its tail (3 ms for 1.5 % of the bins): k_pb_tables is a launch of small workgroups at
//           high occupancy for both, its results a 6 KB table per (UTR, alpha) and a compact [n_log][T][B] table of
//           log-domain values (UTRs with more than PB_LOGCAP such bins: straight into the tensor).  k_phase_b_lin is
//           the matrix path alone and writes EVERY 128-byte line of the tensor exactly once, whole: the log-domain
//           values are merged in from the compact table before the store.  (Form 0's masked stores + later 8-byte
//           stores into the same lines cost 12-14 % extra HBM write traffic: profiles/r02_v4_pmc_WRITE_SIZE.csv.)
//   form 2  k_pb_tables + k_pb_logcol + k_pb_slide (B <= 16, uniform theta grids: every UTR of an ordinary infer_pa
//           run, arange(min_theta, L, theta_step), apa_core.py:940).  On a uniform grid the window tables of all
//           INTERIOR grid points alpha_i - those whose +-3 beta windows are not cut off by the ends of the grid,
//           [c_lo, c_hi] - are one and the same table at a shifted origin: theta_w - theta_i depends on w - i only, and
//           the grid values are integers, so the differences are exact.  k_pb_logcol gathers a log-domain bin's column
//           once for all its windows, k_pb_slide walks all alpha of 16 bins with the window's V rows in an LDS ring.
// Written once and shared: the XCD placement (pb_xcd_slot), the window prologue (pb_windows, pb_weight), the two-pass
// log-sum-exp (pb_window_lse), where a log-domain value goes (pb_store_log), the matrix walk of one alpha
// (pb_matrix_walk) and the reduction of the tile extents (pb_reduce_extents).  k_pb_slide, the tuned kernel of the
// default path, keeps its own placement line and its own finish: with either shared its instructions change.
#define PB_LOGCAP 64

// Workgroup -> (UTR, sub-slot 0 .. blocks_max - 1) for grids of 8 * ceil(n_utr / 8) * blocks_max workgroups.  Blocks b and
// b+8 share an XCD: all workgroups of a UTR go to one XCD so its V rows (each is read by ~43 neighbouring alphas) are
// fetched into one L2 only.  Placement only affects speed.  false: a slot beyond the last UTR.
__device__ __forceinline__ bool pb_xcd_slot(const UtrDesc *__restrict__ descs, int n_utr, int blocks_max, UtrDesc &d, int &sub) {
    const int id = blockIdx.x, slot = id >> 3;
    const int uu = (slot / blocks_max) * 8 + (id & 7);
    if (uu >= n_utr) return false;
    d = descs[uu];
    sub = slot % blocks_max;
    return true;
}

// The +-3 beta windows of alpha = theta_i, by the whole workgroup (barriers inside; the caller's LDS arrays):
// lo / hi [B] the window ends per beta, g [B][Wmax] = log N(theta_w; alpha, beta_j) from lo[j] on, G [B] the window
// normaliser, lo_all / Wall the union window.  err_flag 1: a window wider than Wmax (cut); 2: the union wider than Wmax
// (false is returned, to every thread: the workgroup has nothing to compute).
__device__ __forceinline__ bool pb_windows(const UtrDesc &d, const DevParams &P, const double *th, int i, int Wmax, double *g,
                                           double *G, int *lo, int *hi, int *err_flag, int &lo_all, int &Wall) {
    const int B = P.B, tid = threadIdx.x;
    const double ti = th[i];
    if (tid < B) {     // window of beta_tid: [searchsorted(theta, alpha - 3 beta, left), searchsorted(theta, alpha + 3 beta, right) - 1] (:221-222)
        const double beta = P.betas[tid];
        int a = i, b = i;
        const double lob = ti - 3 * beta, hib = ti + 3 * beta;
        // the walks start from where a uniform grid would put the window's ends and correct in either direction (the
        // grid is ascending, so the boundary is unique): ~6 dependent loads instead of ~40 on the usual grid
        if (d.T > 1) {
            const double step = (i + 1 < d.T) ? th[i + 1] - ti : ti - th[i - 1];
            if (step > 0.0) {
                const double reach = 3 * beta / step;
                const int jump = (reach < 1e6) ? (int)reach : 0;
                a = max(0, i - jump);
                b = min(d.T - 1, i + jump);
            }
        }
        while (a < i && th[a] < lob) ++a;
        while (a > 0 && th[a - 1] >= lob) --a;          // searchsorted(left)
        while (b > i && th[b] > hib) --b;
        while (b + 1 < d.T && th[b + 1] <= hib) ++b;    // searchsorted(right) - 1
        if (b - a + 1 > Wmax) {
            atomicExch(err_flag, 1);
            b = a + Wmax - 1;
        }
        lo[tid] = a;
        hi[tid] = b;
    }
    __syncthreads();
    for (int e = tid; e < B * Wmax; e += blockDim.x) {
        const int j = e / Wmax, w = e - j * Wmax;
        const int tw = lo[j] + w;
        g[e] = (tw <= hi[j]) ? d_logpdf_normal(th[tw], ti, P.betas[j]) : 0.0;
    }
    __syncthreads();
    if (tid < B) {  // call_logp_theta_sum_kernel (:160-169), serial order
        double psum = 0.0;
        const int W = hi[tid] - lo[tid] + 1;
        for (int w = 0; w < W; ++w) psum += exp(g[(size_t)tid * Wmax + w]);
        G[tid] = log(psum);
    }
    __syncthreads();
    lo_all = lo[0];
    int hi_all = hi[0];
    for (int j = 1; j < B; ++j) {
        lo_all = min(lo_all, lo[j]);
        hi_all = max(hi_all, hi[j]);
    }
    Wall = hi_all - lo_all + 1;  // <= Wmax when windows nest (they do: symmetric in value)
    if (Wall > Wmax) {
        if (tid == 0) atomicExch(err_flag, 2);
        return false;
    }
    return true;
}

// exp(g - G) of beta j at tap w relative to lo_all, 0 outside beta j's window: indexed like this the matrix path needs
// no per-beta window test
__device__ __forceinline__ double pb_weight(const double *g, const double *G, const int *lo, const int *hi, int Wmax, int lo_all,
                                            int Wall, int j, int w) {
    const int tw = lo_all + w;
    if (w < Wall && tw >= lo[j] && tw <= hi[j]) return exp(g[(size_t)j * Wmax + (tw - lo[j])] - G[j]);
    return 0.0;
}

// One log-domain value (cal_res_kernel, :172-179): serial max over the window, then the sum of exp(. - max).  A points
// at the bin's entry of the window's first tap, consecutive taps lie `stride` apart; gj is g's row from that tap on.
// Every argument of the exp is <= 0: the table exp of the E-step, 18 instructions instead of ~40.  SUM_UNROLL: taps the
// second pass takes per trip: 2 for the strided gathers from global memory, 4 for k_pb_logcol's LDS column.  These are
// the factors the compiler chose unasked while the loop stood in each kernel; the shared loop it leaves rolled, and
// k_pb_logcol and k_pb_tables are then 9 % slower.
template <int SUM_UNROLL>
__device__ __forceinline__ double pb_window_lse(const double *A, size_t stride, const double *gj, double Gj, int W,
                                                const double2 *exptab) {
    double mx = A[0] + gj[0] - Gj;
    for (int w = 1; w < W; ++w) {
        const double t = A[w * stride] + gj[w] - Gj;
        if (t > mx) mx = t;
    }
    double sum = 0.0;
#pragma unroll SUM_UNROLL
    for (int w = 0; w < W; ++w) sum += d_exp_nonpos(A[w * stride] + gj[w] - Gj - mx, exptab);
    return d_log_pos(sum) + mx;
}

// Where forms 1 and 2 put the value of (alpha i, beta j) of the UTR's q-th log-domain bin n: the compact table
// Mlog[q][i][j], which the matrix-path kernel merges into its whole-line stores, or - more than PB_LOGCAP such bins -
// the tensor itself, and then the tile's extent
__device__ __forceinline__ void pb_store_log(const UtrDesc &d, int B, int i, int j, int q, int n, double val, double *M,
                                             double *Mlog, int32_t *tile_nend) {
    if (d.n_log <= PB_LOGCAP) {
        Mlog[(size_t)d.mlog_off + ((size_t)q * d.T + i) * B + j] = val;
    } else {
        M[(size_t)d.m_off + ((size_t)i * B + j) * d.Np + n] = val;
        if (val != SENT) {
            const int tile = (i * B + j) / TILE_ROWS;
            const int ext = min(d.Np, (n + 1 + 15) & ~15);
            if (tile_nend[d.tile_off + tile] < ext) atomicMax(&tile_nend[d.tile_off + tile], ext);
        }
    }
}

// Tile extents (used by the M-step, mstep.inc: mstep_span): bins are ordered by read start, so each tensor row is finite on a
// prefix of the bins and holds the sentinel (read impossible) on the rest - 35-50 % of all entries.  For every
// TILE_ROWS-row tile the table gets one past the last bin that is finite in ANY of its rows (rounded up to 16): beyond
// it every row of the tile is the sentinel, and the M-step replaces that part of the dot product by SENT * sum(v)
// instead of streaming it.  The B rows of one alpha lie in at most two tiles: tile0 and, from row j_split on, tile0 + 1;
// fin0 / fin1 are a thread's one-past-last finite bins in the two.  By the whole 256-thread workgroup.
__device__ __forceinline__ void pb_reduce_extents(const UtrDesc &d, int tile0, int fin0, int fin1, int32_t *tile_nend) {
    __shared__ int s_fin[2];
    const int tid = threadIdx.x;
    if (tid < 2) s_fin[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        fin0 = max(fin0, __shfl_xor(fin0, off, 64));
        fin1 = max(fin1, __shfl_xor(fin1, off, 64));
    }
    if ((tid & 63) == 0) {
        atomicMax(&s_fin[0], fin0);
        atomicMax(&s_fin[1], fin1);
    }
    __syncthreads();
    if (tid < 2 && s_fin[tid] > 0)
        atomicMax(&tile_nend[d.tile_off + tile0 + tid], min(d.Np, (s_fin[tid] + 15) & ~15));
}

// The matrix path of one alpha, by the whole 256-thread workgroup: out[j][n] = sum_w pm[j][w] * V[lo_all + w][n] is a
// [16 x W] x [W x N] product; on the f64 matrix cores one v_mfma_f64_16x16x4_f64 covers 16 betas (13 used) x 16 bins x
// 4 taps.  A = weights from LDS (pm [16][WP], zero outside a window / beyond B; lane l: beta l&15, tap l>>4), B = V
// straight from global/L2 (lane l: tap l>>4, bin l&15), D lane l reg q: beta (l>>4)+4q, bin l&15.  MERGE (with `merge`,
// form 1): the values of the UTR's log-domain bins, s_ml[j][q] of bin s_ll[q], go into the same whole-line stores.
// fin0 / fin1: see pb_reduce_extents.
template <bool MERGE>
__device__ __forceinline__ void pb_matrix_walk(const UtrDesc &d, int B, const double *__restrict__ r, const double *__restrict__ pa,
                                               const double *Vu, double *Mi, const double *pm, int WP, int lo_all, int Wall,
                                               int j_split, bool merge, const double *s_ml, const int *s_ll, int &fin0,
                                               int &fin1) {
    typedef double v4d __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4, rc = lane & 15;
    const int nblocks = d.Np >> 4;
    // Tap steps whose four rows all exist (lo_all + w0 + 3 <= T - 1) run without a row clamp: the loop body is one
    // pointer add, one load, one LDS read and the MFMA per block of bins; the (at most one) step that reaches past
    // the last grid point clamps its row - its weight is 0 there.  Two blocks of 16 bins share every weight fragment.
    const int steps = (Wall + 3) >> 2;
    const int full = max(0, min(steps, (d.T - lo_all) >> 2));
    const size_t rstep = (size_t)4 * d.Np;
    const double *pw = pm + rc * WP + kq;
    const double *vbase = Vu + (size_t)(lo_all + kq) * d.Np + rc;
    const int n_log = d.n_log;
    // The 16 x 16 result block: row kq + 4q of lane (kq, rc) is beta kq + 4q of bin n.  Written without divergent
    // branches (the logs are taken on every lane, the stores and the extent bookkeeping are predicated): the
    // per-value `if`s of a straightforward version compiled to ~40 exec-mask sequences per block.
    auto finish = [&](int n, const v4d &acc) {
        const bool pad = n >= d.N;
        const int nn = pad ? d.N - 1 : n;
        const bool lin = !pad && isnan(pa[d.bin_off + nn]) && isnan(r[d.bin_off + nn]);   // r-unknown bin: the matrix path's
        const bool mrg = MERGE && merge && !pad && !lin;
        int qi = 0;
        if (mrg)                                   // (rare lanes: 1-2 % of the bins)
            for (int t = 0; t < n_log; ++t)
                if (s_ll[t] == n) qi = t;
        const bool wr = pad || lin || mrg;
        bool f0 = false, f1 = false;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = kq + 4 * q;
            const bool pos = acc[q] > 0.0;
            const double lg = d_log_pos(pos ? acc[q] : 1.0);
            double val = pad ? 0.0 : (pos ? lg : SENT);
            if (mrg && j < B) val = s_ml[j * n_log + qi];
            if (wr && j < B) Mi[(size_t)j * d.Np + n] = val;
            const bool fin = j < B && ((lin && pos) || (mrg && val != SENT));
            f0 |= fin && j < j_split;
            f1 |= fin && j >= j_split;
        }
        fin0 = max(fin0, f0 ? n + 1 : 0);
        fin1 = max(fin1, f1 ? n + 1 : 0);
    };
    int nb = wave;
    for (; nb + 4 < nblocks; nb += 8) {
        const double *v0 = vbase + nb * 16, *v1 = v0 + 64;
        v4d acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
        int st = 0;
        // Four tap steps per trip: their eight V fragments are requested together, then consumed - one wait on the
        // L2 per trip instead of one per step.  (The loop is bound by that latency, not by issue: 8 or 31
        // instructions per MFMA made no difference, batching the loads took 1.3 ms off; the 1-3 steps left over
        // are batched the same way: another 0.5 ms.  Measured and not kept: predicated batches of 4 / 6 / 12 steps
        // (the compiler serialises them), the next pair's first batch requested before this pair's logs and
        // stores (3 wavefronts per SIMD instead of 4: +1.5 ms; held to 4: -0.15 ms), batched loads in the
        // log-domain path and the grid points of the window searches in LDS (registers: 3 wavefronts, +2 ms).)
        auto batch = [&](auto nbc) {
            constexpr int NB = decltype(nbc)::value;
            double b0[NB], b1[NB], av[NB];
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                b0[k] = v0[k * rstep];
                b1[k] = v1[k * rstep];
            }
#pragma unroll
            for (int k = 0; k < NB; ++k) av[k] = pw[4 * (st + k)];
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[k], b0[k], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[k], b1[k], acc1, 0, 0, 0);
            }
            v0 += NB * rstep;
            v1 += NB * rstep;
            st += NB;
        };
        while (st + 4 <= full) batch(std::integral_constant<int, 4>());
        switch (full - st) {
            case 3: batch(std::integral_constant<int, 3>()); break;
            case 2: batch(std::integral_constant<int, 2>()); break;
            case 1: batch(std::integral_constant<int, 1>()); break;
            default: break;
        }
        for (; st < steps; ++st) {
            const int wr = min(lo_all + 4 * st + kq, d.T - 1);
            const double av = pw[4 * st];
            const double *vr = Vu + (size_t)wr * d.Np + nb * 16 + rc;
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, vr[0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, vr[64], acc1, 0, 0, 0);
        }
        finish(nb * 16 + rc, acc0);
        finish(nb * 16 + 64 + rc, acc1);
    }
    for (; nb < nblocks; nb += 4) {
        const double *v0 = vbase + nb * 16;
        v4d acc0 = {0.0, 0.0, 0.0, 0.0};
        int st = 0;
#pragma unroll 4
        for (; st < full; ++st) {
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(pw[4 * st], *v0, acc0, 0, 0, 0);
            v0 += rstep;
        }
        for (; st < steps; ++st) {
            const int wr = min(lo_all + 4 * st + kq, d.T - 1);
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(pw[4 * st], Vu[(size_t)wr * d.Np + nb * 16 + rc], acc0, 0, 0, 0);
        }
        finish(nb * 16 + rc, acc0);
    }
}

// ---- form 0 ------------------------------------------------------------------------------------------------------------
// One workgroup per (UTR, i).  LDS layout (f64): g[B][Wmax] | p[B][Wmax] | G[B] | lo[B] hi[B] (int32 pairs) | pm[16][WP].
// BMAX 16: the matrix path for B <= 16; BMAX 1: any B, one thread per bin.  all_log (the operator seam): every bin of
// the UTR takes the log-domain path, V / r / pa / loglist are not read.
template <int BMAX>
__global__ __launch_bounds__(256, 5) void k_phase_b(const UtrDesc *__restrict__ descs, DevParams P,
                                                 const double *__restrict__ r,
                                                 const double *__restrict__ pa,
                                                 const double *__restrict__ theta,
                                                 const int32_t *__restrict__ loglist,
                                                 const double *__restrict__ AT,
                                                 const double *__restrict__ V,
                                                 double *__restrict__ M, int Wmax, int all_log,
                                                 int *__restrict__ err_flag, int n_utr, int T_max,
                                                 int32_t *__restrict__ tile_nend) {
    extern __shared__ double sm[];
    __shared__ double2 s_exptab[128];
    d_load_exptab(s_exptab, threadIdx.x, 256);
    UtrDesc d;
    int i;
    if (!pb_xcd_slot(descs, n_utr, T_max, d, i) || i >= d.T) return;
    const int B = P.B;
    const int tid = threadIdx.x;
    double *g = sm;                       // [B][Wmax]  logN(theta_w; theta_i, beta_j)
    double *p = sm + (size_t)B * Wmax;    // [B][Wmax]  exp(g - G), 0 outside the window (the one-thread-per-bin path's)
    double *G = p + (size_t)B * Wmax;     // [B]
    int *lo = (int *)(G + B);             // [B]
    int *hi = lo + B;                     // [B]
    const int WP = ((Wmax + 3) & ~3) + 1;                      // odd pitch: conflict-light fragment reads
    double *pm = reinterpret_cast<double *>(hi + B + (B & 1)); // [16][WP]  the same weights as the matrix path's A operand
    int lo_all, Wall;
    if (!pb_windows(d, P, theta + d.theta_off, i, Wmax, g, G, lo, hi, err_flag, lo_all, Wall)) return;
    const bool matrix = !all_log && BMAX == 16;
    if (matrix) {
        for (int e = tid; e < 16 * WP; e += blockDim.x) {
            const int j = e / WP, w = e - j * WP;
            pm[e] = (j < B && w < Wmax) ? pb_weight(g, G, lo, hi, Wmax, lo_all, Wall, j, w) : 0.0;
        }
    } else if (!all_log) {
        for (int e = tid; e < B * Wmax; e += blockDim.x) {
            const int j = e / Wmax, w = e - j * Wmax;
            p[e] = pb_weight(g, G, lo, hi, Wmax, lo_all, Wall, j, w);
        }
    }
    __syncthreads();

    double *Mi = M + (size_t)d.m_off + (size_t)i * B * d.Np;
    const int tile0 = (i * B) / TILE_ROWS, j_split = (tile0 + 1) * TILE_ROWS - i * B;   // rows j >= j_split: tile0 + 1
    int fin0 = 0, fin1 = 0;
    auto note = [&](int j, int n, double val) {
        if (val != SENT) {
            if (j < j_split) fin0 = max(fin0, n + 1);
            else fin1 = max(fin1, n + 1);
        }
    };
    // ---- linear-domain path -----------------------------------------------------------------
    const double *Vu = V + (size_t)d.at_off;
    if (matrix) {
        pb_matrix_walk<false>(d, B, r, pa, Vu, Mi, pm, WP, lo_all, Wall, j_split, false, nullptr, nullptr, fin0, fin1);
    } else if (!all_log) {
        for (int n = tid; n < d.Np; n += blockDim.x) {
            if (n >= d.N) {
                for (int j = 0; j < B; ++j) Mi[(size_t)j * d.Np + n] = 0.0;
                continue;
            }
            if (!isnan(pa[d.bin_off + n]) || !isnan(r[d.bin_off + n])) continue;
            if (B <= BMAX) {
                double acc[BMAX];
#pragma unroll
                for (int j = 0; j < BMAX; ++j) acc[j] = 0.0;
                for (int w = 0; w < Wall; ++w) {
                    const double v = Vu[(size_t)(lo_all + w) * d.Np + n];
#pragma unroll
                    for (int j = 0; j < BMAX; ++j)
                        if (j < B) acc[j] += v * p[(size_t)j * Wmax + w];
                }
#pragma unroll
                for (int j = 0; j < BMAX; ++j)
                    if (j < B) {
                        const double val = (acc[j] > 0.0) ? d_log_pos(acc[j]) : SENT;
                        Mi[(size_t)j * d.Np + n] = val;
                        note(j, n, val);
                    }
            } else {
                for (int j = 0; j < B; ++j) {
                    double acc = 0.0;
                    for (int w = 0; w < Wall; ++w)
                        acc += Vu[(size_t)(lo_all + w) * d.Np + n] * p[(size_t)j * Wmax + w];
                    const double val = (acc > 0.0) ? d_log_pos(acc) : SENT;
                    Mi[(size_t)j * d.Np + n] = val;
                    note(j, n, val);
                }
            }
        }
    } else {
        for (int n = d.N + tid; n < d.Np; n += blockDim.x)
            for (int j = 0; j < B; ++j) Mi[(size_t)j * d.Np + n] = 0.0;
    }
    // ---- log-domain path ----------------------------------------------------------------------
    const int n_log = all_log ? d.N : d.n_log;
    const double *Au = AT + (size_t)d.at_off;
    for (int item = tid; item < n_log * B; item += blockDim.x) {
        const int j = item / n_log, q = item - j * n_log;
        const int n = all_log ? q : loglist[d.log_off + q];
        const double val = pb_window_lse<2>(Au + (size_t)lo[j] * d.Np + n, (size_t)d.Np, g + (size_t)j * Wmax, G[j], hi[j] - lo[j] + 1,
                                         s_exptab);
        Mi[(size_t)j * d.Np + n] = val;
        note(j, n, val);
    }
    if (tile_nend) pb_reduce_extents(d, tile0, fin0, fin1, tile_nend);
}

// ---- forms 1 and 2: the tables ---------------------------------------------------------------------------------------------
// One 128-thread workgroup per (UTR, alpha): the window prologue into the side tables tb_i / tb_G / tb_pm, then - form 1,
// loglist != NULL - the log-domain bins of its alpha, one THREAD per (beta, bin), with g and G still in LDS.
// LDS layout: g[B][Wmax] | G[16] | lo[16] hi[16].
#define PB_TAB_THREADS 128
template <int BMAX>
__global__ __launch_bounds__(PB_TAB_THREADS) void k_pb_tables(const UtrDesc *__restrict__ descs, DevParams P,
                                                  const double *__restrict__ theta, int Wmax, int WP,
                                                  int32_t *__restrict__ tb_i /* [sum T][40]: lo[16] hi[16] lo_all Wall */,
                                                  double *__restrict__ tb_G /* [sum T][16] */,
                                                  double *__restrict__ tb_pm /* [sum T][16][WP] */,
                                                  int *__restrict__ err_flag, int T_max,
                                                  const int32_t *__restrict__ loglist, const double *__restrict__ AT,
                                                  double *__restrict__ M, double *__restrict__ Mlog,
                                                  int32_t *__restrict__ tile_nend) {
    extern __shared__ double sm[];
    __shared__ double2 s_exptab[128];
    d_load_exptab(s_exptab, threadIdx.x, PB_TAB_THREADS);
    const UtrDesc d = descs[blockIdx.y];
    const int i = blockIdx.x;
    if (i >= d.T) return;
    const int B = P.B, tid = threadIdx.x;
    double *g = sm;                        // [B][Wmax]
    double *G = g + (size_t)B * Wmax;      // [16]
    int *lo = (int *)(G + 16);             // [16]
    int *hi = lo + 16;                     // [16]
    if (tid < 16) {                        // the table rows beyond B: empty windows
        lo[tid] = 0;
        hi[tid] = -1;
    }
    __syncthreads();
    int lo_all, Wall;
    if (!pb_windows(d, P, theta + d.theta_off, i, Wmax, g, G, lo, hi, err_flag, lo_all, Wall)) return;
    const size_t row = (size_t)d.theta_off + i;
    if (tid < 16) {
        tb_i[row * 40 + tid] = lo[tid];
        tb_i[row * 40 + 16 + tid] = hi[tid];
        tb_G[row * 16 + tid] = (tid < B) ? G[tid] : 0.0;
    }
    if (tid == 0) {
        tb_i[row * 40 + 32] = lo_all;
        tb_i[row * 40 + 33] = Wall;
    }
    double *pm = tb_pm + row * (size_t)(16 * WP);     // the 16 x WP weight tile of the matrix path
    for (int e = tid; e < 16 * WP; e += blockDim.x) {
        const int j = e / WP, w = e - j * WP;
        pm[e] = (j < B && w < Wmax) ? pb_weight(g, G, lo, hi, Wmax, lo_all, Wall, j, w) : 0.0;
    }
    const int n_log = loglist ? d.n_log : 0;        // loglist == NULL: the log-domain bins are k_pb_logcol's
    const double *Au = AT + (size_t)d.at_off;
    for (int item = tid; item < n_log * B; item += blockDim.x) {     // item (j, q) = beta j, q-th log-domain bin of the UTR
        const int j = item / n_log, q = item - j * n_log;
        const int n = loglist[d.log_off + q];
        const double val = pb_window_lse<2>(Au + (size_t)lo[j] * d.Np + n, (size_t)d.Np, g + (size_t)j * Wmax, G[j], hi[j] - lo[j] + 1,
                                         s_exptab);
        pb_store_log(d, B, i, j, q, n, val, M, Mlog, tile_nend);
    }
}

// ---- form 1: the matrix path per alpha -------------------------------------------------------------------------------------
// LDS layout: pm[16][WP] | s_ml[16][PB_LOGCAP] | s_ll[PB_LOGCAP], staged from k_pb_tables' tables.
__global__ __launch_bounds__(256, 5) void k_phase_b_lin(const UtrDesc *__restrict__ descs, DevParams P,
                                                         const double *__restrict__ r, const double *__restrict__ pa,
                                                         const int32_t *__restrict__ loglist, const double *__restrict__ V,
                                                         double *__restrict__ M, const double *__restrict__ Mlog,
                                                         int WP, const int32_t *__restrict__ tb_i,
                                                         const double *__restrict__ tb_pm, int n_utr, int T_max,
                                                         int32_t *__restrict__ tile_nend) {
    extern __shared__ double sm[];
    UtrDesc d;
    int i;
    if (!pb_xcd_slot(descs, n_utr, T_max, d, i) || i >= d.T) return;
    const int B = P.B, tid = threadIdx.x;
    double *pm = sm;                                  // [16][WP]
    double *s_ml = pm + 16 * WP;                      // [B][n_log] values of this alpha's log-domain bins (n_log <= PB_LOGCAP)
    int *s_ll = (int *)(s_ml + 16 * PB_LOGCAP);       // [PB_LOGCAP] their bin numbers
    const size_t row = (size_t)d.theta_off + i;
    const bool merge = d.n_log > 0 && d.n_log <= PB_LOGCAP;
    {
        const double *src = tb_pm + row * (size_t)(16 * WP);
        for (int e = tid; e < 16 * WP; e += 256) pm[e] = src[e];
        if (merge) {
            for (int e = tid; e < B * d.n_log; e += 256) {       // s_ml[j][q] <- Mlog[q][i][j]
                const int j = e / d.n_log, q = e - j * d.n_log;
                s_ml[e] = Mlog[(size_t)d.mlog_off + ((size_t)q * d.T + i) * B + j];
            }
            if (tid < d.n_log) s_ll[tid] = loglist[d.log_off + tid];
        }
    }
    const int lo_all = tb_i[row * 40 + 32], Wall = tb_i[row * 40 + 33];
    __syncthreads();
    const int tile0 = (i * B) / TILE_ROWS, j_split = (tile0 + 1) * TILE_ROWS - i * B;
    int fin0 = 0, fin1 = 0;
    pb_matrix_walk<true>(d, B, r, pa, V + (size_t)d.at_off, M + (size_t)d.m_off + (size_t)i * B * d.Np, pm, WP, lo_all, Wall, j_split,
                         merge, s_ml, s_ll, fin0, fin1);
    if (tile_nend) pb_reduce_extents(d, tile0, fin0, fin1, tile_nend);
}

// ---- form 2 ------------------------------------------------------------------------------------------------------------
//   k_pb_logcol  one workgroup per (UTR, log-domain bin): the bin's column A[:, n] is gathered into LDS ONCE (T strided
//                8-byte reads) and serves all T x B window sums of that bin - k_phase_b / k_pb_tables fetch the same column
//                entries again for every (alpha, beta) window they fall into, 8 bytes of a 128-byte line at a time, which kept
//                the texture addresser busy for 8 of k_pb_tables' 10 ms.  log N(theta_w; alpha, beta) comes from a
//                [B][window] table of the interior point c_lo, the normaliser G[i][j] from k_pb_tables.
//   k_pb_slide   one WAVEFRONT per (UTR, block of 16 bins) walks ALL alpha: the window's V rows of its 16 bins live in a
//                private 64-row ring in LDS - every V value is fetched from L2 once, not once per window it belongs to
//                (43 times) - rows enter four at a time, one group ahead of need.  Interior alpha take the weight tile
//                from the workgroup's LDS copy of the canonical table, the others from k_pb_tables' per-alpha tables
//                (fragments requested one alpha ahead).  No barrier after the first: a wavefront shares nothing it writes.
//                The 16 x 16 result block is finished as in pb_matrix_walk (whole-line stores, log-domain bins merged
//                in; their values for alpha i + 1 are requested while alpha i is multiplied).
__global__ __launch_bounds__(256) void k_pb_logcol(const UtrDesc *__restrict__ descs, DevParams P, const double *__restrict__ theta,
                                                   const int32_t *__restrict__ loglist, const int32_t *__restrict__ logbin_utr,
                                                   const double *__restrict__ AT, const int32_t *__restrict__ tb_i,
                                                   const double *__restrict__ tb_G, double *__restrict__ M,
                                                   double *__restrict__ Mlog, int32_t *__restrict__ tile_nend, int Wmax) {
    extern __shared__ double sm[];
    __shared__ double2 s_exptab[128];
    d_load_exptab(s_exptab, threadIdx.x, 256);
    const UtrDesc d = descs[logbin_utr[blockIdx.x]];
    const int q = (int)((int64_t)blockIdx.x - d.log_off), n = loglist[blockIdx.x];
    const int B = P.B, T = d.T, tid = threadIdx.x;
    double *Acol = sm;                          // [T]
    double *grel = Acol + ((T + 1) & ~1);       // [B][Wmax]: log N(theta_w; theta_c, beta_j) for w in beta_j's window at the interior point c
    int *cj = (int *)(grel + (size_t)B * Wmax); // [16] c - lo_c[j]
    const double *th = theta + d.theta_off;
    const double *Au = AT + (size_t)d.at_off;
    const int c = d.c_lo;
    const size_t crow = (size_t)d.theta_off + c;
    for (int t = tid; t < T; t += 256) Acol[t] = Au[(size_t)t * d.Np + n];
    for (int e = tid; e < B * Wmax; e += 256) {
        const int j = e / Wmax, w = e - j * Wmax;
        const int a = tb_i[crow * 40 + j], b = tb_i[crow * 40 + 16 + j];
        grel[e] = (a + w <= b) ? d_logpdf_normal(th[a + w], th[c], P.betas[j]) : 0.0;
    }
    if (tid < B) cj[tid] = c - tb_i[crow * 40 + tid];
    __syncthreads();
    // items beta-major: the lanes of a wavefront share beta, hence (away from the grid's ends) the window length - alpha-major
    // they ran 13 different lengths side by side, every lane for the longest (3 ... 43 taps: 55 % of the lanes' steps were idle)
    for (int item = tid; item < T * B; item += 256) {
        const int j = item / T, i = item - j * T;
        const size_t row = (size_t)d.theta_off + i;
        const int a = tb_i[row * 40 + j], W = tb_i[row * 40 + 16 + j] - a + 1;
        const double *gj = grel + (size_t)j * Wmax + (a - i + cj[j]);     // tap a + w sits at offset (a + w) - i from alpha
        const double val = pb_window_lse<4>(Acol + a, 1, gj, tb_G[row * 16 + j], W, s_exptab);
        pb_store_log(d, B, i, j, q, n, val, M, Mlog, tile_nend);
    }
}

#define PB_RING 64          // V rows per wavefront ring (>= widest window + 3 + two groups of 4 ahead)
#define PB_STEPS 12         // tap steps of 4 a window may take (W_max <= 48)
// k_pb_slide, second form (round 3).  The first form took 10.8 ms for 512 UTRs where its f64 work is 5; timing-only builds (no log:
// -3.2 ms, no MFMA: -2.2 ms, a quarter of the stores: -0.6 ms, all three: 5.1 ms LEFT) showed a loop bound by its own round trips:
// one global load waited for with vmcnt(0) on every alpha, an LDS read waited for in front of each of the 12 dependent MFMAs,
// a branch per tap step, the weights fetched through flat loads because an LDS and a global pointer shared a variable.  Now:
//   - interior alpha are walked FOUR AT A TIME in straight-line code: the V group a block needs was requested a block earlier,
//     the interior weights sit in registers for the whole walk, all ring reads of an alpha are in flight before its first MFMA,
//     the four logarithms of a lane are independent chains;
//   - edge alpha (their own weight tables from k_pb_tables, windows cut off by the grid's ends) keep a per-alpha loop with the
//     same ring discipline; rows beyond the grid and tap steps beyond a window meet zero weights, the ring is zeroed first so
//     that whatever they read is finite.
// Same taps in the same (step, k) places of the same MFMA chain as k_phase_b_lin / the first form: identical bits.
__global__ __launch_bounds__(256, 4) void k_pb_slide(const UtrDesc *__restrict__ descs, DevParams P,
                                                      const double *__restrict__ r, const double *__restrict__ pa,
                                                      const int32_t *__restrict__ loglist, const double *__restrict__ V,
                                                      double *__restrict__ M, const double *__restrict__ Mlog,
                                                      int WP, const int32_t *__restrict__ tb_i,
                                                      const double *__restrict__ tb_pm, int n_utr, int blocks_max,
                                                      int32_t *__restrict__ tile_nend) {
    extern __shared__ double sm[];
    typedef double v4d __attribute__((ext_vector_type(4)));
    const int id = blockIdx.x, slot = id >> 3;
    const int uu = (slot / blocks_max) * 8 + (id & 7);      // blocks b and b+8 share an XCD: a UTR's bin blocks meet in one L2
    if (uu >= n_utr) return;
    const UtrDesc d = descs[uu];
    const int bb = slot % blocks_max;
    if (64 * bb >= d.Np) return;
    const int B = P.B, T = d.T, tid = threadIdx.x;
    double *pmc = sm;                                  // [16][WP]: the interior points' weight tile
    double *rings = pmc + 16 * WP;                     // [4][PB_RING][16]
    const size_t crow = (size_t)d.theta_off + d.c_lo;
    for (int e = tid; e < 16 * WP; e += 256) pmc[e] = tb_pm[crow * (size_t)(16 * WP) + e];
    const int lo_off = d.c_lo - tb_i[crow * 40 + 32], Wall_c = tb_i[crow * 40 + 33];
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, kq = lane >> 4, rc = lane & 15;
    const int n0 = 64 * bb + 16 * wave, n = n0 + rc;
    if (n0 >= d.Np) return;                            // (no barrier below)
    double *ring = rings + wave * (PB_RING * 16);
#pragma unroll
    for (int e = 0; e < PB_RING * 16 / 64; ++e) ring[64 * e + lane] = 0.0;
    const double *Vu = V + (size_t)d.at_off;
    // what kind of bin this lane finishes - the same for every alpha
    const bool pad = n >= d.N;
    const int nn = pad ? d.N - 1 : n;
    const bool lin = !pad && isnan(pa[d.bin_off + nn]) && isnan(r[d.bin_off + nn]);
    const int n_log = d.n_log;
    const bool mrg = n_log > 0 && n_log <= PB_LOGCAP && !pad && !lin;
    int qi = 0;
    if (mrg)
        for (int t = 0; t < n_log; ++t)
            if (loglist[d.log_off + t] == n) qi = t;
    const bool wr = pad || lin || mrg;
    const double *ml = Mlog + (size_t)d.mlog_off + (size_t)qi * T * B;       // [i][j] of this lane's log-domain bin
    // log-domain values are merged in by the wavefronts that have such a bin (about one in five); the others walk without the
    // loads and without the waits the compiler puts in front of their use (vmcnt(0): every store of the walk so far)
    const bool wave_mrg = __ballot(mrg) != 0ull;
    auto load_merge = [&](int i, double (&m)[4], auto mw) {                  // the lane's four log-domain values of alpha i
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) m[q4] = 0.0;
        if constexpr (decltype(mw)::value) {
            if (mrg && i < T)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4)
                    if (kq + 4 * q4 < B) m[q4] = ml[(size_t)i * B + kq + 4 * q4];
        }
    };
    double mcur[4], mnext[4];
    load_merge(0, mcur, std::bool_constant<true>());
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) asm volatile("" : "+v"(mcur[q4]));   // arrived before the walk: no load pending on mcur at a loop header
    // ring: rows enter in aligned groups of 4 (lane (kq, rc): row 4 g + kq, bin n0 + rc).  have(gq) makes the groups up to gq
    // readable and keeps the next one in flight: it is written into the ring when a later call needs it, not before
    const unsigned lane_off = (unsigned)(kq * d.Np + n);          // (row kq, bin n) of a 4-row group / a 4-beta group of one alpha
    auto load_group = [&](int g4) -> double {
        const double *Vg = Vu + (size_t)(4 * g4) * d.Np;             // uniform base + lane offset
        return (4 * g4 + kq < T) ? Vg[lane_off] : 0.0;               // beyond the grid: weight 0 there, the value must only be finite
    };
    auto put_group = [&](int g4, double v) { ring[((4 * g4 + kq) & (PB_RING - 1)) * 16 + rc] = v; };
    int next_g4 = 0, pend_g = -1;
    double pend = 0.0;
    auto have = [&](int gq) {
        if (pend_g >= 0 && pend_g <= gq) {
            put_group(pend_g, pend);
            pend_g = -1;
        }
        while (next_g4 <= gq) {                          // (only at the start of the walk: later the group is already there)
            put_group(next_g4, load_group(next_g4));
            ++next_g4;
        }
        if (pend_g < 0) {
            pend = load_group(next_g4);
            pend_g = next_g4;
            ++next_g4;
        }
    };
    // tile extents: finite bins per 64-row tile, flushed when the walk leaves a tile
    int cur_tile = 0, fin0 = 0, fin1 = 0;
    auto flush = [&](int tile, int fin) {              // max over the wavefront on DPP (fin >= 0), complete in lane 63
        fin = max(fin, __builtin_amdgcn_update_dpp(0, fin, 0x111, 0xf, 0xf, false));     // row_shr:1
        fin = max(fin, __builtin_amdgcn_update_dpp(0, fin, 0x112, 0xf, 0xf, false));     // row_shr:2
        fin = max(fin, __builtin_amdgcn_update_dpp(0, fin, 0x114, 0xf, 0xf, false));     // row_shr:4
        fin = max(fin, __builtin_amdgcn_update_dpp(0, fin, 0x118, 0xf, 0xf, false));     // row_shr:8: lane 15 of a row has the row's max
        fin = max(fin, __builtin_amdgcn_update_dpp(0, fin, 0x142, 0xa, 0xf, false));     // row_bcast:15 into rows 1 and 3
        fin = max(fin, __builtin_amdgcn_update_dpp(0, fin, 0x143, 0xc, 0xf, false));     // row_bcast:31 into rows 2 and 3
        if (lane == 63 && fin > 0) atomicMax(&tile_nend[d.tile_off + tile], min(d.Np, (fin + 15) & ~15));
    };
    // finish the 16 x 16 block of alpha i: rows kq + 4 q4 = beta, column = this lane's bin (as k_phase_b_lin)
    auto finish = [&](int i, const v4d &acc, const double (&mc)[4], auto mw) {
        constexpr bool MW = decltype(mw)::value;
        double *Mi = M + (size_t)d.m_off + (size_t)i * B * d.Np;    // uniform
        const int tile0 = (i * B) / TILE_ROWS, j_split = (tile0 + 1) * TILE_ROWS - i * B;
        if (tile0 != cur_tile) {                         // the walk has left cur_tile for good (tile0 = cur_tile + 1)
            flush(cur_tile, fin0);
            fin0 = fin1;
            fin1 = 0;
            cur_tile = tile0;
        }
        double lg[4];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) lg[q4] = d_log_pos(acc[q4] > 0.0 ? acc[q4] : 1.0);
        bool f0 = false, f1 = false;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int j = kq + 4 * q4;
            const bool pos = acc[q4] > 0.0;
            double val = pad ? 0.0 : (pos ? lg[q4] : SENT);
            if (MW && mrg) val = mc[q4];
            if (wr && j < B) (Mi + (size_t)(4 * q4) * d.Np)[lane_off] = val;
            const bool fin = j < B && ((lin && pos) || (MW && mrg && val != SENT));
            f0 |= fin && j < j_split;
            f1 |= fin && j >= j_split;
        }
        fin0 = max(fin0, f0 ? n + 1 : 0);
        fin1 = max(fin1, f1 ? n + 1 : 0);
    };
    // ring entry of this lane for tap step st of the current alpha: row (lo_all + 4 st + kq) mod PB_RING; lo_all moves by whole
    // rows from alpha to alpha, so the entries advance by (delta x 16) mod ring size
    unsigned roff = (unsigned)(kq * 16 + rc);           // tap step 0; step st sits 4 rows = 64 entries further
    int lo_prev = 0;
    // an alpha with its own weight table (k_pb_tables' output): the grid's ends, and what the blocks of four leave over
    auto edge_alpha = [&](int i, auto mw) {
        const size_t row = (size_t)d.theta_off + i;
        const int lo_all = tb_i[row * 40 + 32], Wall = tb_i[row * 40 + 33];
        const double *pwg = tb_pm + row * (size_t)(16 * WP) + rc * WP + kq;
        const int steps = (Wall + 3) >> 2;
        double av[PB_STEPS];
#pragma unroll
        for (int st = 0; st < PB_STEPS; ++st) av[st] = (st < steps) ? pwg[4 * st] : 0.0;
        load_merge(i + 1, mnext, mw);
        have((lo_all + 4 * steps - 1) >> 2);
        const unsigned adv = (unsigned)(lo_all - lo_prev) * 16u;
        lo_prev = lo_all;
        double rv[PB_STEPS];
        roff += adv;
#pragma unroll
        for (int st = 0; st < PB_STEPS; ++st) rv[st] = ring[(roff + 64u * st) & (PB_RING * 16 - 1)];
        v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int st = 0; st < PB_STEPS; ++st)
            if (st < steps) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st], rv[st], acc, 0, 0, 0);
        finish(i, acc, mcur, mw);
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) mcur[q4] = mnext[q4];
    };
    // four interior alpha: weights w[] in registers, one row further per alpha
    auto canon_block = [&](int i0, auto ns, const double (&w)[PB_STEPS], auto mw) {
        constexpr int NS = decltype(ns)::value;
        have((i0 + 3 - lo_off + 4 * NS - 1) >> 2);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int i = i0 + a;
            load_merge(i + 1, mnext, mw);
            const int lo_all = i - lo_off;
            const unsigned adv = (unsigned)(lo_all - lo_prev) * 16u;
            lo_prev = lo_all;
            double rv[NS];
            roff += adv;
#pragma unroll
            for (int st = 0; st < NS; ++st) rv[st] = ring[(roff + 64u * st) & (PB_RING * 16 - 1)];
            v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int st = 0; st < NS; ++st) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(w[st], rv[st], acc, 0, 0, 0);
            finish(i, acc, mcur, mw);
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) mcur[q4] = mnext[q4];
        }
    };
    const int steps_c = (Wall_c + 3) >> 2;
    auto walk = [&](auto mw) {
        int i = 0;
        const int head = min(d.c_lo, T);
        for (; i < head; ++i) edge_alpha(i, mw);
        if (i + 3 <= d.c_hi) {
            double w[PB_STEPS];
            const double *pw = pmc + rc * WP + kq;
#pragma unroll
            for (int st = 0; st < PB_STEPS; ++st) w[st] = (st < steps_c) ? pw[4 * st] : 0.0;
            if (steps_c <= PB_STEPS - 1)
                for (; i + 3 <= d.c_hi; i += 4) canon_block(i, std::integral_constant<int, PB_STEPS - 1>(), w, mw);
            else
                for (; i + 3 <= d.c_hi; i += 4) canon_block(i, std::integral_constant<int, PB_STEPS>(), w, mw);
        }
        for (; i < T; ++i) edge_alpha(i, mw);
    };
    if (wave_mrg) walk(std::bool_constant<true>());
    else walk(std::bool_constant<false>());
    flush(cur_tile, fin0);
    flush(cur_tile + 1, fin1);
}
