// mstep_multi.inc - k4_mstep: k3_mstep's LDS-DMA stream (mstep_ring.inc) with the per-tile set-up and arg-max epilogue
// taken off the critical path.  (included by scape_hip.hip after mstep_ring.inc; same inputs, same per-(job, tile)
// outputs, same frame (mstep.inc) and same MFMA chain per score: identical bits.)  The headline kernel.
//
// Why (profiles/README.md, round 3: no-stream / no-MFMA / no-DMA timing builds of k3_mstep): a tile's set-up - job scan,
// window / support reductions, suffix-sum look-ups: five to six dependent global round trips - and its arg-max epilogue
// took 0.32 ms of a 3.0 ms launch in the early rounds and 0.25 of 1.95 ms in the late ones, during which the workgroup
// neither streams nor multiplies; the late rounds stream at the memory system's limit otherwise.  Here one workgroup owns
// M4_TPW consecutive tiles of a UTR:
//   - ONE set-up for all of them: the UTR's job descriptors are read once, every tile's job list is compacted from
//     registers, and the four wavefronts finish one tile's table each (window, support, v offset, output slot and the
//     constant part c0 of every job's scores) into LDS - later tiles start from LDS, not from global memory;
//   - DMA roles balanced: wavefronts 0-1 request the 8 tile pieces of a half-chunk (4 each), wavefronts 2-3 the even / odd
//     job-vector pieces (one per running column group each): issuing a piece costs a wavefront 100-200 cycles, and with
//     all vector pieces on one wavefront (k3_mstep) that wavefront's 6-8 pieces per half-chunk set the pace of the four;
//   - tile i + 1's first ring slots are requested as soon as tile i's last k-step has been multiplied, BEFORE tile i's
//     arg-max epilogue, which works from LDS tables and an exchange area of its own: no round trip, the DMA latency of
//     the next tile hides behind it.
// "Job" here is an M-step COLUMN: the list entries are column ids (job * depth + slot, em_lockstep.inc), a job that ran
// ahead has up to EM_DEPTH of them in a launch, each with its own v vector, window and partial table.
// A tile that holds more jobs than one pass (> 64: rare at one round per pass; in a call that runs ahead 40-57 % of the
// tiles of passes 0-4, by a CPU trace of the headline stream) gets its further passes at the end, one after the other, each
// with a scan and table of its own.  Calls with few live tiles (job lists cut into passes for several workgroups,
// gridDim.y > 1) run k3_mstep instead (the host picks the kernel).

#ifndef M4_TPW
#define M4_TPW 2                      // tiles per workgroup (<= 4: one wavefront finishes one tile's table); measured: 2 -> 1.96 ms per launch, 3 -> 2.01, 4 -> 2.02 (k3_mstep: 2.07)
#endif
static_assert(M4_TPW >= 1 && M4_TPW <= 4, "one wavefront per tile table");
#define M4_NW 4                       // wavefronts per workgroup, all of them MFMA wavefronts; 0-1 also request the tile pieces, 2-3 the job vectors
#define M4_WPC M3_WPC                 // workgroups per CU
// (Measured and dropped, see DESIGN.md section 3 - the code is in the history: extra loader wavefronts (4 at 2 workgroups per CU:
// 2.26 ms per launch; 2 at 3 workgroups per CU, 96 VGPRs: 2.41 ms, against 1.98), fragment prefetch, s_setprio, a third / fourth
// tile per workgroup, the tile ring deeper than the vector ring.)
static_assert(M4_TPW * M4_NW <= 16 && M4_NW == 4, "per-wavefront hit counts of the set-up (mstep_ordinal: 4 per tile)");
__device__ __forceinline__ bool m4_is_tile_issuer(int wave) { return wave < 2; }
__device__ __forceinline__ bool m4_is_vec_issuer(int wave) { return wave >= 2; }
__device__ __forceinline__ int m4_role_index(int wave) { return wave & 1; }   // 0 / 1 within the role
// LDS: [ring area | exchange 4 x 64 x (f64 + i32) | per tile: 64 x {lo, hi, ptoff, voff16 (i32), c0 (f64)} | per tile 8 ints | 4 u64]
#define M4_REC_BYTES (64 * 24)
#define M4_TAIL_BYTES (4 * 64 * 12 + M4_TPW * (M4_REC_BYTES + 12 * 4) + 16 * 4 + 4 * 8)
#define M4_AREA_BYTES (((M4_WPC >= 3 ? 53760 : 81920) - M4_TAIL_BYTES) / 1024 * 1024)
#define M4_LDS_BYTES (M4_AREA_BYTES + M4_TAIL_BYTES)
static_assert((M4_LDS_BYTES + 1279) / 1280 * M4_WPC <= 128, "LDS granules: the rings do not fit at this occupancy");
// Ring depths per G (16-job column groups of the pass): the job vectors must be requested as far ahead as the tiles.
// They are L2 hits, but a CU's vector-memory pipeline returns in issue order, so a vector piece comes back behind every
// tile piece - HBM misses - requested before it: in-loop cycle stamps (-DM4_STAMPS) showed the vector wavefronts waiting
// 3,700 cycles per half-chunk for pieces requested ONE half-chunk ahead (5,500 cycles) at 3 running groups, and the tile
// wavefronts waiting for them at the barrier, with the tile ring three deep.  So: as many (tile slot + vector slot) pairs
// as fit, a left-over tile slot if there is room for one.
__host__ __device__ constexpr int m4_rv(int G) { return M4_AREA_BYTES / (G * 2048 + 8192) < 2 ? 2 : M4_AREA_BYTES / (G * 2048 + 8192); }
__host__ __device__ constexpr int m4_rt(int G) {
    return (M4_AREA_BYTES - m4_rv(G) * G * 2048) / 8192 > 10 ? 10 : (M4_AREA_BYTES - m4_rv(G) * G * 2048) / 8192;
}
static_assert(m4_rt(4) >= 2 && m4_rt(3) >= 2 && m4_rt(2) >= 2 && m4_rt(1) >= 2, "a ring needs the slot being multiplied and one in flight");

struct M4Tile {          // what a wavefront needs to stream one tile (registers / scalars)
    const double *tb0, *vb0;          // uniform bases: Mu + row0 Np + n_lo, V + n_lo
    int nh, G, np_w;                  // half-chunks, column groups, this wavefront's tile pieces per half-chunk
    int he1, he2, he3;                // half-chunks column groups 1, 2, 3 run for (group 0 runs all nh): jobs are sorted by where their v ends
    unsigned pieces;                  // their piece numbers, 4 bits each
    bool needed;                      // this wavefront's 16 rows are inside some job's window
    unsigned offs[4];                 // DMA source offsets: wavefronts 0-1 tile pieces, wavefronts 2-3 one job-vector piece per column group
#ifdef M4_STAMPS
    unsigned long long *stamps;       // tools-only: [4 GA][2 roles][4] cycle sums + [8] iteration counts
#endif
};

// column groups still running at half-chunk h (group 0 runs all nh; he1 >= he2 >= he3)
template <int G>
__device__ __forceinline__ int m4_gact(const M4Tile &T, int h) {
    int g = 1;
    if (G > 1 && h < T.he1) g = 2;
    if (G > 2 && h < T.he2) g = 3;
    if (G > 3 && h < T.he3) g = 4;
    return g;
}
template <int G>
__device__ __forceinline__ void m4_issue(const M4Tile &T, unsigned lds_area, int wave, int h) {
    constexpr int RT = m4_rt(G), RV = m4_rv(G), VSLOT = G * 16 * M3_CH;
    if (m4_is_vec_issuer(wave)) {      // two wavefronts: the even / odd 8-job pieces of the job vectors
        const double *b = T.vb0 + (size_t)h * M3_CH;
        const unsigned dst = lds_area + (unsigned)(h % RV) * (VSLOT * 8) + (unsigned)m4_role_index(wave) * 1024u;
        const int np = m4_gact<G>(T, h);               // one piece of each running group per vector wavefront
#pragma unroll
        for (int q = 0; q < G; ++q)
            if (q < np) m3_dma<false>(T.offs[q], b, dst + (unsigned)q * 2048u);
    } else if (m4_is_tile_issuer(wave)) {   // two wavefronts: tile pieces 0-3 / 4-7 (8 rows x 128 B each)
        const double *b = T.tb0 + (size_t)h * M3_CH;
        const unsigned dst = lds_area + RV * VSLOT * 8 + (unsigned)(h % RT) * (M3_TSLOT * 8);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < T.np_w) m3_dma<M3_TILE_NT>(T.offs[i], b, dst + ((T.pieces >> (4 * i)) & 15u) * 1024u);
    }
}
// the first ring slots of a tile (the ring is empty: every wavefront has passed the barrier behind the previous tile's last k-step)
template <int G>
__device__ __forceinline__ void m4_prologue(const M4Tile &T, unsigned lds_area, int wave) {
    const int ahead = m4_is_vec_issuer(wave) ? m4_rv(G) - 1 : m4_rt(G) - 1;
    for (int j = 0; j < ahead; ++j)
        if (j < T.nh) m4_issue<G>(T, lds_area, wave, j);
}
// half-chunks [h0, h1) of a tile with GA of its G column groups still running (ring layout: G's)
template <int G, int GA>
__device__ __forceinline__ void m4_seg(const M4Tile &T, unsigned lds_area, const double *area, int wave, int lane, int h0, int h1,
                                       v4f64 (&acc)[MT_MAXJ / 16]) {
    constexpr int RT = m4_rt(G), RV = m4_rv(G), VSLOT = G * 16 * M3_CH;
    const double *ringV = area, *ringT = area + RV * VSLOT;
    const int kq = lane >> 4, rc = lane & 15;
    int offd[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) offd[s] = m3_frag_index(s, kq, rc);
    const bool vwave = m4_is_vec_issuer(wave);
    const int ahead = vwave ? RV - 1 : RT - 1;
    const int nh = T.nh;
#ifdef M4_STAMPS   // tools-only: where a half-chunk iteration's cycles go, per wavefront role (sums over the launch)
    unsigned long long st_wait = 0, st_bar = 0, st_issue = 0, st_mfma = 0;
#define M4_T(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#else
#define M4_T(v)
#endif
    for (int h = h0; h < h1; ++h) {
        M4_T(t0);
        const int keep = min(ahead - 1, nh - 1 - h);      // younger slots of this wavefront's ring: they stay in flight
        int younger = T.np_w * keep;                       // ... = this many DMA pieces
        if (vwave) {                                       // (the vector wavefront's pieces per slot shrink as groups drop out)
            younger = 0;
            for (int y = 1; y <= keep; ++y) younger += m4_gact<G>(T, h + y);
        }
        // (a wavefront's two epilogue stores of the previous tile may sit among the younger operations: the count is then
        // a little stricter than needed for the first half-chunk of a tile, never laxer)
        m3_wait_vm(younger);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        M4_T(t1);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        M4_T(t2);
        if (h + ahead < nh) m4_issue<G>(T, lds_area, wave, h + ahead);
        M4_T(t3);
        if (T.needed) {
            const double *ts = ringT + (h % RT) * M3_TSLOT + (16 * wave + rc) * M3_CH;
            const double *vs = ringV + (h % RV) * VSLOT + rc * M3_CH;
            mstep_kstep<GA>(ts, vs, offd, acc);
        }
#ifdef M4_STAMPS
        asm volatile("" : "+v"(acc[0]));          // the last MFMA's result is waited for before the stamp
        M4_T(t4);
        st_wait += t1 - t0;
        st_bar += t2 - t1;
        st_issue += t3 - t2;
        st_mfma += t4 - t3;
#endif
    }
#ifdef M4_STAMPS
    if (lane == 0 && h1 > h0) {
        unsigned long long *sp = T.stamps + 4 * ((GA - 1) * 2 + (vwave ? 1 : 0));     // by running groups and wavefront role
        atomicAdd(&sp[0], st_wait);
        atomicAdd(&sp[1], st_bar);
        atomicAdd(&sp[2], st_issue);
        atomicAdd(&sp[3], st_mfma);
        atomicAdd(T.stamps + 32 + (GA - 1) * 2 + (vwave ? 1 : 0), (unsigned long long)(h1 - h0));
    }
#endif
#undef M4_T
}
// the whole tile: the column groups drop out of the stream one after the other (jobs are sorted by where their v ends)
template <int G>
__device__ __forceinline__ void m4_loop(const M4Tile &T, unsigned lds_area, const double *area, int wave, int lane,
                                        v4f64 (&acc)[MT_MAXJ / 16]) {
    const int nh = T.nh;
    int h = 0;
    if constexpr (G >= 4) {
        m4_seg<G, 4>(T, lds_area, area, wave, lane, h, min(T.he3, nh), acc);
        h = max(h, min(T.he3, nh));
    }
    if constexpr (G >= 3) {
        m4_seg<G, 3>(T, lds_area, area, wave, lane, h, min(T.he2, nh), acc);
        h = max(h, min(T.he2, nh));
    }
    if constexpr (G >= 2) {
        m4_seg<G, 2>(T, lds_area, area, wave, lane, h, min(T.he1, nh), acc);
        h = max(h, min(T.he1, nh));
    }
    m4_seg<G, 1>(T, lds_area, area, wave, lane, h, nh, acc);
}

__global__ __launch_bounds__(64 * M4_NW, (M4_NW * M4_WPC + 3) / 4) void k4_mstep(MSTEP_PARAMS(groups_max)) {
    extern __shared__ __attribute__((aligned(16))) double m4_lds[];
    double *area = m4_lds;
    double *x_ps = m4_lds + M4_AREA_BYTES / 8;                        // exchange [4][64] scores
    int *x_pr = reinterpret_cast<int *>(x_ps + 4 * 64);               // exchange [4][64] rows
    int *rec_i = x_pr + 4 * 64;                                       // per tile: [64][6 ints]: lo, hi, ptoff, voff16, c0 (2 ints)
    int *t_sc = rec_i + M4_TPW * 64 * 6;                              // per tile: cnt, n_lo, nh, need, first, n_ext, job count overflow, -
    int *t_he = t_sc + M4_TPW * 8;                                    // per tile: half-chunks the 4 column groups run for
    int *s_misc = t_he + M4_TPW * 4;                                  // [0..3] per-wave hit counts
    unsigned long long *s_by = reinterpret_cast<unsigned long long *>(s_misc + 16);
    const unsigned lds_area = (unsigned)(size_t)(__attribute__((address_space(3))) double *)area;

    int ul, tg;
    if (!mstep_block(blockIdx.x, n_utr, groups_max, ul, tg)) return;
    const int u = active[ul];
    const UtrDesc d = descs[u];
    const int B = P.B, Np = d.Np;
    const int nrows = d.T * B;
    const int t_first = tg * M4_TPW;
    if (t_first * MT_ROWS >= nrows) return;
    const int n_tiles = min(M4_TPW, (nrows - t_first * MT_ROWS + MT_ROWS - 1) / MT_ROWS);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double *Mu = M + (size_t)d.m_off;
    const int64_t jlo = ujob_off[u], jhi = ujob_off[u + 1];

    // ---- set-up, part 1: the job lists of tiles [i_lo, i_hi), compacted in job-list order from one read of the job
    // windows; of a tile's hits those with ordinals [base, base + 64) go into its table (field 2 = job id for now)
    int found[M4_TPW];
    auto collect = [&](int i_lo, int i_hi, int base) {
#pragma unroll
        for (int i = 0; i < M4_TPW; ++i) found[i] = 0;
        for (int64_t j0 = jlo; j0 < jhi; j0 += 64 * M4_NW) {
            const int64_t jj = j0 + tid;
            int j = -1, lo = 0, hi = 0;
            if (jj < jhi) {
                j = ujob_list[jj];
                if (rd_m[j]) {
                    lo = rd_lo[j];
                    hi = rd_hi[j];
                }
            }
#pragma unroll
            for (int i = 0; i < M4_TPW; ++i) {
                const int row0 = (t_first + i) * MT_ROWS;
                const bool hit = i >= i_lo && i < i_hi && lo < row0 + MT_ROWS && hi > row0;     // (lo = hi = 0 never hits)
                mstep_count_hits(hit, lane, wave, s_misc + M4_NW * i);
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < M4_TPW; ++i) {
                const int row0 = (t_first + i) * MT_ROWS;
                const bool hit = i >= i_lo && i < i_hi && lo < row0 + MT_ROWS && hi > row0;
                const int off = mstep_ordinal(__ballot(hit), lane, wave, s_misc + M4_NW * i, found[i]);
                if (hit && off >= base && off < base + 64) rec_i[(i * 64 + off - base) * 6 + 2] = j;
            }
            __syncthreads();
        }
    };
    // ---- set-up, part 2: one wavefront finishes tile i's table (lanes = job slots) -------------------------------------
    auto finish_table = [&](int i, int total, int base) {
        const int t = t_first + i, row0 = t * MT_ROWS;
        const int cnt = max(0, min(total - base, 64));
        const int n_ext = tile_nend[d.tile_off + t];
        MstepWin w;
        int j = 0, lo = 0, hi = 0, n0 = 0, n1 = 0, po32 = 0, vo16 = 0;
        double c0 = 0.0;
        if (lane < cnt) {
            j = rec_i[(i * 64 + lane) * 6 + 2];
            lo = rd_lo[j];
            hi = rd_hi[j];
            n0 = rd_n0[j];
            n1 = rd_n1[j];
            const int64_t vo = voff[j];
            const double lw = rd_lw[j], sv = rd_sv[j];
            const int64_t po = ptoff[j];
            c0 = mstep_c0(lw, sv, Vsuf[mstep_tail_index(vo, j, n_ext)]);
            w = mstep_window_of_job(lo, hi, n0, n1, row0, t);
            po32 = (int)(po + t);              // output slot of this (job, tile)
            vo16 = (int)(vo >> 4);
        }
        w = mstep_window_reduce(w);
        const MstepSpan sp = mstep_span(w.nlo, w.nhi, Np, n_ext);
        // Terms with v[n] == 0 add exactly 0 to a score, so a job's columns need no k-steps beyond the last bin of its v.
        // Jobs are ranked by that end, longest first, and take their table slots in rank order: column group g (ranks
        // 16 g ..) then runs only he_g = the end of its first member, in half-chunks - the groups drop out of the
        // stream one after the other (13 % fewer MFMAs in round 0, 7-9 % in rounds 1-25: profiles/README.md).
        // Which slot a job gets changes nothing in its own chain of MFMAs.
        if (lane < 4) t_he[i * 4 + lane] = 0;
        int hc = 0;                                       // half-chunks this job's v reaches into the streamed range
        if (lane < cnt && n1 > n0) hc = max(0, min((min(n1, sp.n_hi) - sp.n_lo + 15) >> 4, sp.nh));
        int rank = 0;
        for (int o = 0; o < 64; ++o) {
            const int other = __shfl(hc, o, 64);
            rank += (o < cnt) && (other > hc || (other == hc && o < lane));
        }
        if (lane < cnt) {
            int *rc_ = rec_i + (i * 64 + rank) * 6;
            rc_[0] = lo;
            rc_[1] = hi;
            rc_[2] = po32;
            rc_[3] = vo16;
            *reinterpret_cast<double *>(rc_ + 4) = c0;
            if ((rank & 15) == 0) t_he[i * 4 + (rank >> 4)] = hc;
        }
        if (lane == 0) {
            int *sc = t_sc + i * 8;
            sc[0] = cnt;
            sc[1] = sp.n_lo;
            sc[2] = sp.nh;
            sc[3] = w.mk;
            sc[4] = w.first;
            sc[5] = n_ext;
            sc[6] = total;
        }
    };
    collect(0, n_tiles, 0);
    if (wave < n_tiles) {
        int total = 0;
#pragma unroll
        for (int i = 0; i < M4_TPW; ++i)
            if (i == wave) total = found[i];
        finish_table(wave, total, 0);
    }
    if (tid == 0) s_by[0] = s_by[1] = s_by[2] = 0ull;
    __syncthreads();

    const int l8 = lane >> 3, u8 = lane & 7;
    auto make_tile = [&](int i, M4Tile &T) {
        const int t = t_first + i, row0 = t * MT_ROWS;
        const int *sc = t_sc + i * 8;
        const int cnt = __builtin_amdgcn_readfirstlane(sc[0]), n_lo = __builtin_amdgcn_readfirstlane(sc[1]);
        const int need = __builtin_amdgcn_readfirstlane(sc[3]);
        T.nh = __builtin_amdgcn_readfirstlane(sc[2]);
        T.G = (cnt + 15) >> 4;
        T.he1 = __builtin_amdgcn_readfirstlane(t_he[i * 4 + 1]);
        T.he2 = __builtin_amdgcn_readfirstlane(t_he[i * 4 + 2]);
        T.he3 = __builtin_amdgcn_readfirstlane(t_he[i * 4 + 3]);
        T.needed = (need >> wave) & 1;
        T.np_w = 0;
        T.pieces = 0;
        if (cnt == 0) T.nh = 0;
        if (m4_is_tile_issuer(wave)) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int pc = 4 * m4_role_index(wave) + q;  // tile piece: rows 8 pc .. 8 pc + 7
                if ((need >> (pc >> 1)) & 1) {
                    const int r = 8 * pc + l8;
                    const int rr = min(row0 + r, nrows - 1) - row0;
                    const unsigned o = (unsigned)(((size_t)rr * Np + m3_src_unit(r, u8)) * 8);
                    // compact the needed pieces to the front (np_w is wave-uniform: `need` is)
                    if (T.np_w == 0) T.offs[0] = o; else if (T.np_w == 1) T.offs[1] = o; else if (T.np_w == 2) T.offs[2] = o; else T.offs[3] = o;
                    T.pieces |= (unsigned)pc << (4 * T.np_w);
                    ++T.np_w;
                }
            }
        } else if (m4_is_vec_issuer(wave)) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int js = 8 * (2 * q + m4_role_index(wave)) + l8;      // job slots of this wavefront's piece of column group q
                const unsigned vo16 = (unsigned)rec_i[(i * 64 + min(js, max(cnt, 1) - 1)) * 6 + 3];
                T.offs[q] = (unsigned)((((size_t)vo16 << 4) + m3_src_unit(js, u8)) * 8);
            }
        }
#ifdef M4_STAMPS
        T.stamps = counters + (4 + 5 * 64 + 16);
#endif
        T.tb0 = m3_uniform_ptr(Mu + (size_t)row0 * Np + n_lo);
        T.vb0 = m3_uniform_ptr(V + n_lo);
        if (tid == 0 && T.nh > 0) mstep_tally(s_by, need, nrows, row0, T.nh, cnt, sc[4]);
    };
#define M4_BY_G(G_, CALL)                 \
    switch (G_) {                          \
        case 0: break;                     \
        case 1: { constexpr int GG = 1; CALL; } break; \
        case 2: { constexpr int GG = 2; CALL; } break; \
        case 3: { constexpr int GG = 3; CALL; } break; \
        default: { constexpr int GG = 4; CALL; } break; \
    }
    // one (tile, pass): the stream of `cur` (its first slots are already requested), then - before the arg-max epilogue -
    // the first slots of the next one, if there is one and its table is ready
    auto process = [&](int i, M4Tile &cur, bool have_next, int i_next, M4Tile &nxt) {
        const int t = t_first + i, row0 = t * MT_ROWS;
        v4f64 acc[MT_MAXJ / 16];
#pragma unroll
        for (int g = 0; g < MT_MAXJ / 16; ++g) acc[g] = (v4f64){0.0, 0.0, 0.0, 0.0};
        M4_BY_G(cur.G, m4_loop<GG>(cur, lds_area, area, wave, lane, acc));
        // every wavefront has multiplied its last k-step: the ring is free for the next tile's first slots
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (have_next) {
            make_tile(i_next, nxt);
            M4_BY_G(nxt.G, m4_prologue<GG>(nxt, lds_area, wave));
        }
        const int cnt = __builtin_amdgcn_readfirstlane(t_sc[i * 8]);
        const int G = (cnt + 15) >> 4;
        const int kq = lane >> 4, rc = lane & 15;
#pragma unroll
        for (int g = 0; g < MT_MAXJ / 16; ++g) {
            if (g < G) {
                const int slot_j = 16 * g + rc;
                MstepBest b;
                if (slot_j < cnt) {
                    const int *rc_ = rec_i + (i * 64 + slot_j) * 6;
                    const int lo = rc_[0], hi = rc_[1];
                    const double c0 = *reinterpret_cast<const double *>(rc_ + 4);
                    b = mstep_best_of_rows(b, acc[g], c0, lo, hi, row0 + 16 * wave + kq, nrows);
                }
                b = mstep_merge_lanes(b);
                if (kq == 0 && slot_j < cnt) {
                    x_ps[wave * 64 + slot_j] = b.score;
                    x_pr[wave * 64 + slot_j] = b.row;
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (tid < cnt) {         // wavefront 0 (cnt <= 64)
            const MstepBest b = mstep_merge_waves(x_ps, x_pr, 64, tid);
            const int *rc_ = rec_i + (i * 64 + tid) * 6;
            // ptoff + t fits 32 bits (the host checks the size of the partial tables)
            pt_score[(unsigned)rc_[2]] = b.score;
            pt_row[(unsigned)rc_[2]] = mstep_row_or_fallback(b.row, rc_[0], row0);
        }
        // (the exchange area is rewritten by the next epilogue only behind a later barrier)
    };
    M4Tile cur, nxt;
    make_tile(0, cur);
    M4_BY_G(cur.G, m4_prologue<GG>(cur, lds_area, wave));
    bool overflow = false;
    for (int i = 0; i < n_tiles; ++i) {
        process(i, cur, i + 1 < n_tiles, i + 1, nxt);
        overflow |= t_sc[i * 8 + 6] > 64;
        cur = nxt;
    }
    // tiles with more than 64 jobs (common in the first passes of a call that runs ahead): their further passes one after the other, each with its own scan and table
    if (overflow) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();
        for (int i = 0; i < n_tiles; ++i) {
            const int total = __builtin_amdgcn_readfirstlane(t_sc[i * 8 + 6]);
            for (int base = 64; base < total; base += 64) {
                collect(i, i + 1, base);
                if (wave == 0) finish_table(i, total, base);
                __syncthreads();
                make_tile(i, cur);
                M4_BY_G(cur.G, m4_prologue<GG>(cur, lds_area, wave));
                process(i, cur, false, 0, nxt);
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0) t_sc[i * 8 + 6] = total;      // (finish_table keeps it; explicit for the next pass)
                __syncthreads();
            }
        }
    }
#undef M4_BY_G
    if (tid == 0) mstep_tally_flush(counters, s_by);
}
