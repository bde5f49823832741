// mstep.inc - the frame the three M-step kernels share (included by scape_hip.hip after em_lockstep.inc and before
// mstep_staged.inc: k2_mstep, mstep_ring.inc: k3_mstep, mstep_multi.inc: k4_mstep).
//
// The grid arg-max M-step (max_alpha_beta, apa_core.py:507-523): one workgroup per (UTR, MT_ROWS-row tile of the [T*B, N]
// tensor) computes D[rows x jobs] = Mtile[rows x n] * V[n x jobs] on the f64 matrix cores and writes, per (job, tile), the
// first maximum of the job's window inside the tile to a partial table that the next k2_estep reduces in row order.
// The kernels differ in how the two operands reach the matrix cores (their stream); everything around the stream is
// here, once: which (UTR, tile) a block takes, the stable compaction of a tile's job list, the window and support
// reduction of a pass, the constant part of a job's scores, the byte tally, the arg-max and its merges, and the two
// halves of the LDS swizzle with the k-step of the DMA kernels.  The three kernels must return identical bits: apart
// from the MFMA chains of the streams, every floating-point operation and comparison they apply to a score is here.
// (With run-ahead the entries of ujob_list are COLUMNS - job * depth + slot, one v vector, window and partial table
// each - and every per-"job" array of the kernels is indexed by column; "job" reads "column".)
// The pure integer rules are __host__ __device__: tools/mstep_frame_check.cpp drives them, and the scalar cores of the
// first-maximum rule, on the CPU against plain restatements.
// No function here holds a barrier or a wait except mstep_collect, which k4_mstep does not call: k4 synchronises with
// s_waitcnt lgkmcnt(0) + s_barrier so that the next tile's DMAs stay in flight across its epilogue.

typedef double v4f64 __attribute__((ext_vector_type(4)));    // the D fragment of v_mfma_f64_16x16x4_f64
#define M3_CH 16                       // bins per half-chunk of the DMA kernels' streams

// The parameters of all three kernels (launch_mstep passes them); EXTENT names the second grid factor: the tiles of
// the largest UTR, for k4_mstep its tile groups.  k2_mstep and k3_mstep take jobs_per_pass and dbg behind them.
#define MSTEP_PARAMS(EXTENT)                                                                                               \
    const UtrDesc *__restrict__ descs, DevParams P, const double *__restrict__ M, const int32_t *__restrict__ active,      \
        int n_utr, int EXTENT, const int64_t *__restrict__ ujob_off, const int32_t *__restrict__ ujob_list,                \
        const double *__restrict__ V, const double *__restrict__ Vsuf, const int64_t *__restrict__ voff,                   \
        const int32_t *__restrict__ rd_m, const int32_t *__restrict__ rd_lo, const int32_t *__restrict__ rd_hi,            \
        const double *__restrict__ rd_lw, const double *__restrict__ rd_sv, const int32_t *__restrict__ rd_n0,             \
        const int32_t *__restrict__ rd_n1, const int64_t *__restrict__ ptoff, double *__restrict__ pt_score,               \
        int32_t *__restrict__ pt_row, const int32_t *__restrict__ tile_nend, unsigned long long *__restrict__ counters

// ---- the grid ------------------------------------------------------------------------------------------------------
// Block id -> (UTR ul of the call's active list, tile or tile group t < extent); false: the block has nothing to do.
// The grid is ((n_utr + 7) / 8) * 8 * extent blocks (launch_mstep).  Blocks b and b + 8 share an XCD (its L2): one XCD
// gets all tiles of a UTR, so the job vectors (V, ~1 MB per UTR) are fetched into one L2 only.  With fewer than 8 UTRs
// in the call that rule would leave XCDs idle: the tiles are then dealt round-robin.  Placement only affects speed.
__host__ __device__ inline bool mstep_block(int id, int n_utr, int extent, int &ul, int &t) {
    if (n_utr >= 8) {
        const int slot = id >> 3;
        ul = (slot / extent) * 8 + (id & 7);
        t = slot % extent;
    } else {
        ul = id % n_utr;
        t = id / n_utr;
    }
    return ul < n_utr && t < extent;
}

// ---- the job list of a tile: a stable compaction, 256 list entries per trip and one per thread -----------------------
// (stable: the workgroups that share a tile when gridDim.y > 1 must agree on which jobs belong to which pass)
// First half of a trip: the wavefront's hits, counted into wcnt[wave].  A barrier follows in the caller.
__device__ __forceinline__ unsigned long long mstep_count_hits(bool hit, int lane, int wave, int *wcnt) {
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) wcnt[wave] = __popcll(mask);
    return mask;
}
// Second half: the ordinal of this thread's entry among the tile's hits (meaningful where it is a hit), given the hits
// `found` before this trip; `found` moves on to the end of the trip.  A barrier follows before wcnt is written again.
__device__ __forceinline__ int mstep_ordinal(unsigned long long mask, int lane, int wave, const int *wcnt, int &found) {
    int off = found;
    for (int w = 0; w < wave; ++w) off += wcnt[w];
    off += __popcll(mask & ((1ull << lane) - 1ull));
    found += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    return off;
}
// The whole scan of k2_mstep / k3_mstep (one tile per workgroup; both barriers of a trip are here): store(ordinal, job)
// for every job of list entries [jlo, jhi) whose window covers rows [row0, row0 + MT_ROWS); returns their number, the
// same in every thread.
template <class Store>
__device__ __forceinline__ int mstep_collect(const int32_t *__restrict__ ujob_list, int64_t jlo, int64_t jhi,
                                             const int32_t *__restrict__ rd_m, const int32_t *__restrict__ rd_lo,
                                             const int32_t *__restrict__ rd_hi, int row0, int tid, int lane, int wave, int *wcnt,
                                             Store &&store) {
    int found = 0;
    for (int64_t j0 = jlo; j0 < jhi; j0 += 256) {
        const int64_t jj = j0 + tid;
        int j = -1;
        bool hit = false;
        if (jj < jhi) {
            j = ujob_list[jj];
            hit = rd_m[j] && rd_lo[j] < row0 + MT_ROWS && rd_hi[j] > row0;
        }
        const unsigned long long mask = mstep_count_hits(hit, lane, wave, wcnt);
        __syncthreads();
        const int off = mstep_ordinal(mask, lane, wave, wcnt, found);
        if (hit) store(off, j);
        __syncthreads();
    }
    return found;
}

// ---- the window and support of a pass ------------------------------------------------------------------------------
struct MstepWin {
    int mk = 0;              // which of the tile's four 16-row groups some job's window touches (bit g4)
    int nlo = 0x7fffffff;    // the union of the bins where some job's v is not exactly 0: [nlo, nhi), nhi = 0: empty
    int nhi = 0;
    int first = 0;           // jobs whose window starts in this tile
};
// one job: window rows [lo, hi), v != 0 only inside bins [n0, n1); tile t = rows row0 ..
__host__ __device__ inline MstepWin mstep_window_of_job(int lo, int hi, int n0, int n1, int row0, int t) {
    MstepWin w;
    for (int g4 = 0; g4 < 4; ++g4) w.mk |= (lo - row0 < 16 * (g4 + 1) && hi - row0 > 16 * g4) ? (1 << g4) : 0;
    if (n1 > n0) {
        w.nlo = n0;
        w.nhi = n1;
    }
    w.first = lo / MT_ROWS == t;
    return w;
}
// over the jobs of a pass, one per lane of a wavefront (lanes without a job pass MstepWin{}); identical in every lane
__device__ __forceinline__ MstepWin mstep_window_reduce(MstepWin w) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        w.mk |= __shfl_xor(w.mk, off, 64);
        w.nlo = min(w.nlo, __shfl_xor(w.nlo, off, 64));
        w.nhi = max(w.nhi, __shfl_xor(w.nhi, off, 64));
    }
    w.first = __popcll(__ballot(w.first != 0));
    return w;
}
// The bins a pass streams: terms with v[n] == 0 add exactly 0 to every score, so only the union of the supports, and
// beyond n_ext = the tile's finite extent every row of the tile holds the sentinel (k_tile_extent): that part of each
// dot product is SENT * sum_{n >= n_ext} v[n], no tensor bytes needed.  In half-chunks of 16 bins: [n_lo, n_hi), nh of them.
struct MstepSpan {
    int n_lo, n_hi, nh;
};
__host__ __device__ inline MstepSpan mstep_span(int nlo, int nhi, int Np, int n_ext) {
    const int n_lo = (nhi > 0) ? (nlo & ~15) : 0;
    const int n_up = (nhi + 15) & ~15;
    const int n_sup = (nhi > 0) ? (Np < n_up ? Np : n_up) : 0;
    const int n_hi = n_sup < n_ext ? n_sup : n_ext;
    return MstepSpan{n_lo, n_hi, (n_hi > n_lo) ? (n_hi - n_lo) >> 4 : 0};
}
// where Vsuf holds sum_{n >= n_ext} v_j[n] (estep_body: column j's suffix sums start at (voff[j] >> 4) + j)
__host__ __device__ inline int64_t mstep_tail_index(int64_t vo, int j, int n_ext) { return (vo >> 4) + j + (n_ext >> 4); }
// The part of a job's scores that does not depend on the row: score(a, b) = sum_n (log w_k + M[a,b,n]) v[n] is evaluated
// as log w_k * sum_n v[n] + sum_n M v, and of the second sum the bins beyond the tile's extent are SENT * tl.
// One fused multiply-add onto the (separately rounded) sentinel product - what all three kernels were compiled to
// when each wrote the expression out under the compiler's default contraction; stated here so that it is no accident.
__host__ __device__ inline double mstep_c0(double lw, double sv, double tl) {
    return __builtin_fma(lw, sv, (tl != 0.0) ? SENT * tl : 0.0);
}

// ---- byte tally ----------------------------------------------------------------------------------------------------
// Bytes a workgroup asks the memory system for (thread 0 keeps the tally in by[0..2], in LDS: the streams have no
// register to spare): tensor-tile bytes (each live tile is read by exactly one workgroup per pass: HBM traffic), the v
// vectors as requested (every tile of a UTR re-reads them: L2 hits after the first) and the v bytes counted once per
// job.  One pass of nh > 0 half-chunks over cnt jobs, `first` of which start in this tile.
__device__ __forceinline__ void mstep_tally(unsigned long long *by, int need, int nrows, int row0, int nh, int cnt, int first) {
    int rows = 0;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4)
        if ((need >> g4) & 1) rows += max(0, min(16, nrows - row0 - 16 * g4));
    const unsigned long long span = (unsigned long long)nh * (M3_CH * 8ull);
    by[0] += span * (unsigned long long)rows;
    by[1] += span * (unsigned long long)cnt;
    by[2] += span * (unsigned long long)first;
}
__device__ __forceinline__ void mstep_tally_flush(unsigned long long *__restrict__ counters, const unsigned long long *by) {
    if (!by[0]) return;
    const int sh = (int)(blockIdx.x & 63);      // 64-way sharded, as the E-step's counters
    atomicAdd(&counters[CNT_MSTEP_TENSOR + sh], by[0]);
    atomicAdd(&counters[CNT_MSTEP_VREQ + sh], by[1]);
    atomicAdd(&counters[CNT_MSTEP_VUNI + sh], by[2]);
}
// SCAPE_HIP_DEBUG: the tile histogram of k2_mstep / k3_mstep (one thread per tile; em_debug_round prints it)
__device__ __forceinline__ void mstep_debug_tile(unsigned long long *dbg, int total) {
    atomicAdd(&dbg[0], 1ull);
    atomicAdd(&dbg[1], (unsigned long long)(total > 0));
    atomicAdd(&dbg[2], (unsigned long long)total);
    atomicAdd(&dbg[3], (unsigned long long)((total + MT_MAXJ - 1) / MT_MAXJ));
    atomicAdd(&dbg[4 + min((total + 15) / 16, 11)], 1ull);
}

// ---- the arg-max: first maximum = lowest row ---------------------------------------------------------------------------
struct MstepBest {
    double score = -INFINITY;
    int row = 0x7fffffff;    // no row of the window seen yet
};
// does (score, row) replace b?  Candidates in ascending row order: strict > keeps the first maximum ...
__host__ __device__ inline bool mstep_beats(double score, const MstepBest &b) { return score > b.score; }
// ... in any order: a tie goes to the lower row
__host__ __device__ inline bool mstep_beats_tied(double score, int row, const MstepBest &b) {
    return score > b.score || (score == b.score && row < b.row);
}
// One lane's four rows of a D fragment (rows row_first + 4 i, ascending) for one job: constant part c0, window [lo, hi).
__host__ __device__ inline MstepBest mstep_best_of_rows(MstepBest b, const v4f64 &acc_g, double c0, int lo, int hi, int row_first,
                                                        int nrows) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = row_first + 4 * i;
        const double sc = c0 + acc_g[i];
        if (row >= lo && row < hi && row < nrows && mstep_beats(sc, b)) {
            b.score = sc;
            b.row = row;
        }
    }
    return b;
}
// over the four lanes (l, l + 16, l + 32, l + 48) that hold a job's 16 rows of a wavefront; identical in all four
__device__ __forceinline__ MstepBest mstep_merge_lanes(MstepBest b) {
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
        const double ob = __shfl_xor(b.score, off, 64);
        const int orr = __shfl_xor(b.row, off, 64);
        if (mstep_beats_tied(ob, orr, b)) {
            b.score = ob;
            b.row = orr;
        }
    }
    return b;
}
// over the wavefronts' results for job slot sj in the exchange arrays ([4][stride]; wavefronts hold ascending rows)
__host__ __device__ inline MstepBest mstep_merge_waves(const double *ps, const int *pr, int stride, int sj) {
    MstepBest b;
    b.score = ps[sj];
    b.row = pr[sj];
    for (int w = 1; w < 4; ++w)
        if (mstep_beats(ps[w * stride + sj], b)) {
            b.score = ps[w * stride + sj];
            b.row = pr[w * stride + sj];
        }
    return b;
}
// the row a (job, tile) entry reports: no row of the window scored (a window that misses the tile's live rows) -> the
// window's first row inside the tile
__host__ __device__ inline int mstep_row_or_fallback(int best_r, int lo, int row0) {
    return (best_r == 0x7fffffff) ? (lo > row0 ? lo : row0) : best_r;
}

// ---- the LDS image of the DMA kernels (k3_mstep, k4_mstep) -----------------------------------------------------------
// A slot row is 16 bins = 8 units of 16 B.  An LDS-DMA instruction writes 1 KB lane-linear, so the bank-conflict-free
// image is made on the SOURCE side: the lane that writes unit u8 of slot row r (a tile row of the tile, or a job slot
// of the pass) fetches the f64 pair starting at bin m3_src_unit(r, u8) of that row's half-chunk ...
__host__ __device__ inline int m3_src_unit(int r, int u8) { return 2 * (u8 ^ ((r >> 1) & 7)); }
// ... and the MFMA fragment lane (kq, rc) finds bin 4 s + kq of slot row 16 w + rc at this f64 index of the row.
// Fragment reads (ds_read_b64) of 16 rows x 2 taps then hit 32 distinct bank pairs.
__host__ __device__ inline int m3_frag_index(int s, int kq, int rc) { return (((2 * s + (kq >> 1)) ^ ((rc >> 1) & 7)) << 1) | (kq & 1); }
// The four k-steps of a half-chunk: ts / vs = this lane's row of the tile slot / of column group 0 of the vector slot,
// offd[s] = m3_frag_index(s, ..); 1 + GA fragment reads, then GA MFMAs per k-step.
template <int GA>
__device__ __forceinline__ void mstep_kstep(const double *ts, const double *vs, const int (&offd)[4], v4f64 (&acc)[MT_MAXJ / 16]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const double a = ts[offd[s]];
        double b[GA];
#pragma unroll
        for (int g = 0; g < GA; ++g) b[g] = vs[g * 16 * M3_CH + offd[s]];
#ifdef M3_NO_MFMA   // tools-only timing build: fragment reads without the matrix instructions (results are wrong)
#pragma unroll
        for (int g = 0; g < GA; ++g) acc[g][0] += a + b[g];
#else
#pragma unroll
        for (int g = 0; g < GA; ++g) acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[g], acc[g], 0, 0, 0);
#endif
    }
}
