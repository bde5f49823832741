// mstep_ring.inc - k3_mstep: the M-step with both MFMA operands brought into LDS by LDS-DMA.
// (included by scape_hip.hip after mstep.inc and mstep_staged.inc; same grid, same job tables, same per-(job, tile)
// outputs as k2_mstep through the same frame (mstep.inc), and the same MFMA chain per score -
// v_mfma_f64_16x16x4_f64 over ascending bins - so the bits are k2_mstep's.)  Runs small calls whose tiles are shared
// by several workgroups (gridDim.y > 1), under SCAPE_HIP_MSTEP=v3 and under SCAPE_HIP_DEBUG.
//
// What changed against k2_mstep, and why (profiles/r02_mstep_per_round.txt: rounds 0-8 ran at 3.5-4.1 TB/s):
// k2_mstep stages every 16 KB tile chunk and its job vectors global -> VGPR -> LDS (ds_write_b128: 13 cycles of
// the CU's LDS store path per KB and wavefront, two barriers per chunk, 48 staging registers).  Here
//   - global_load_lds_dwordx4 writes LDS directly (no staging registers, no ds_write pass);
//   - the stream advances in half-chunks of 16 bins: a tile slot is 64 rows x 128 B, a job-vector slot 64 job
//     columns x 128 B, both 8 KB; rings of M3_RT tile slots and M3_RV vector slots;
//   - ONE barrier per half-chunk: wait (counted vmcnt) for this wavefront's own DMAs of half-chunk h, barrier,
//     then issue the DMAs that refill the slots half-chunk h-1 has just left, then the 4 k-steps of h;
//   - an LDS-DMA instruction writes 1 KB lane-linear (wave-uniform base + 16 B x lane), so the bank-conflict-free
//     image is made on the SOURCE side (m3_src_unit / m3_frag_index, mstep.inc; cdna_hip_programming.md section 5,
//     "Async global->LDS copy");
//   - DMA roles: wavefronts 0-2 issue the 8 tile pieces of a half-chunk (3 + 3 + 2; a piece = 8 rows x 128 B), wavefront 3
//     issues all job-vector pieces (2 per column group).  s_waitcnt vmcnt counts a wavefront's vector-memory operations
//     IN ISSUE ORDER, so a wavefront that issued both kinds could only keep what it issued after its newest vector piece
//     in flight - the first build of this kernel did that and drained its tile ring to one slot at every barrier.  With
//     the roles split, the wait for half-chunk h leaves all min(RT - 2, nh - 1 - h) younger tile slots in flight
//     (vmcnt(pieces per slot x that)), and the vector wavefront its RV - 2 younger slots.

#ifndef M3_WPC
#define M3_WPC 3      // workgroups per CU the kernel is built for
#endif
#ifndef M3_TILE_NT
#define M3_TILE_NT true
#endif
#define M3_TSLOT (64 * M3_CH)          // f64 per tile slot (8 KB)
// LDS of a workgroup: [ring area | s_jobs[64] | s_tail[64] f64 | 16 ints | 4 u64].  gfx950 hands LDS out in granules of
// 1,280 B (160 KB = 128 granules): 3 workgroups per CU get 42 granules = 53,760 B each, 2 get 64 = 81,920 B.
// (The first build of this kernel asked for 54,112 B and silently ran 2 workgroups per CU.)
#define M3_TAIL_BYTES (64 * 4 + 64 * 8 + 16 * 4 + 4 * 8)
#define M3_AREA_BYTES (M3_WPC >= 3 ? 51 * 1024 : 78 * 1024)
#define M3_LDS_BYTES (M3_AREA_BYTES + M3_TAIL_BYTES)
static_assert((M3_LDS_BYTES + 1279) / 1280 * M3_WPC <= 128, "LDS granules: the rings do not fit at this occupancy");
// The ring area is split per pass by the number G of 16-job column groups: a job-vector slot holds 16 G job columns x
// 128 B (2 G KB), RV of them; the rest goes to 8-KB tile slots.  Passes with few jobs - the late, HBM-bound rounds - get
// the deeper tile ring (more bytes in flight), passes with 3-4 groups are co-bound by the matrix cores anyway.
__host__ __device__ constexpr int m3_rv(int G) { return (M3_WPC >= 3) ? (G <= 1 ? 3 : 2) : 3; }
__host__ __device__ constexpr int m3_rt(int G) {
    return (M3_AREA_BYTES - m3_rv(G) * G * 2048) / 8192 > 10 ? 10 : (M3_AREA_BYTES - m3_rv(G) * G * 2048) / 8192;
}
static_assert(m3_rt(4) > m3_rv(4) && m3_rt(1) > m3_rv(1), "the vmcnt accounting assumes the tile ring is the deeper one");

// one 1-KB LDS-DMA piece: lane l writes LDS bytes [lds_dst + 16 l, +16) from sbase + off_bytes(l).
// M0 carries the LDS base and is saved/restored inside the statement (the compiler reserves it);
// the leading s_nop covers a base or destination SGPR that a v_readfirstlane has just written.
// NT: non-temporal policy for bytes that are read once per launch (the tensor tiles): they need not displace the job
// vectors, which every tile of a UTR re-reads, from the XCD's L2 (MI355X_MICROARCH.md, row nt-weights).
template <bool NT>
__device__ __forceinline__ void m3_dma(unsigned off_bytes, const double *sbase, unsigned lds_dst) {
#ifdef M3_NO_DMA   // tools-only timing build: the MFMA loop on whatever LDS holds (results are wrong)
    return;
#endif
    unsigned keep;
    if constexpr (NT)
        asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(off_bytes), "s"(sbase), "s"(lds_dst)
                     : "memory");
    else
        asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(off_bytes), "s"(sbase), "s"(lds_dst)
                     : "memory");
}
__device__ __forceinline__ void m3_wait_vm(int n) {   // n is wave-uniform
#define M3_W(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
    switch (n) {
        M3_W(0) M3_W(1) M3_W(2) M3_W(3) M3_W(4) M3_W(5) M3_W(6) M3_W(7) M3_W(8) M3_W(9) M3_W(10) M3_W(11) M3_W(12)
        M3_W(13) M3_W(14) M3_W(15) M3_W(16) M3_W(17) M3_W(18) M3_W(19) M3_W(20) M3_W(21) M3_W(22) M3_W(23) M3_W(24)
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
#undef M3_W
}
__device__ __forceinline__ const double *m3_uniform_ptr(const double *p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return reinterpret_cast<const double *>(((unsigned long long)hi << 32) | lo);
}

// the stream of one pass: G column groups of 16 jobs, nh half-chunks starting at bin n_lo.
// offs: this wavefront's DMA source offsets - wavefronts 0-2: tile pieces 3 w .. (rows 8 p + lane / 8), np_w of them in
// offs[0 .. 2] with their piece numbers in `pieces` (4 bits each); wavefront 3: job-vector pieces 0 .. 2 G - 1.
template <int G>
__device__ __forceinline__ void m3_stream(const double *tb0 /* Mu + row0 Np + n_lo, uniform */, const double *vb0 /* V + n_lo, uniform */,
                                          unsigned lds_area, const double *area, int nh,
                                          int wave, int lane, bool needed, const unsigned (&offs)[8], int np_w, unsigned pieces,
                                          v4f64 (&acc)[MT_MAXJ / 16]) {
    constexpr int RT = m3_rt(G), RV = m3_rv(G);
    constexpr int VSLOT = G * 16 * M3_CH;                 // f64 per job-vector slot
    const double *ringV = area, *ringT = area + RV * VSLOT;
    const unsigned lds_V = lds_area, lds_T = lds_area + RV * VSLOT * 8;
    const int kq = lane >> 4, rc = lane & 15;
    int offd[4];   // f64 index inside a 16-bin row of the swizzled image, per k-step
#pragma unroll
    for (int s = 0; s < 4; ++s) offd[s] = m3_frag_index(s, kq, rc);
    const bool vwave = wave == 3;
    auto issue = [&](int h) {          // this wavefront's pieces of half-chunk h (tile pieces, or all job-vector pieces)
        if (vwave) {
            const double *b = vb0 + (size_t)h * M3_CH;
            const unsigned dst = lds_V + (unsigned)(h % RV) * (VSLOT * 8);
#pragma unroll
            for (int i = 0; i < 2 * G; ++i) m3_dma<false>(offs[i], b, dst + (unsigned)i * 1024u);
        } else {
            const double *b = tb0 + (size_t)h * M3_CH;
            const unsigned dst = lds_T + (unsigned)(h % RT) * (M3_TSLOT * 8);
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if (i < np_w) m3_dma<M3_TILE_NT>(offs[i], b, dst + ((pieces >> (4 * i)) & 15u) * 1024u);
        }
    };
    // the vector wavefront runs RV - 1 half-chunks ahead, the tile wavefronts RT - 1
    const int ahead = vwave ? RV - 1 : RT - 1, per = vwave ? 2 * G : np_w;
    for (int j = 0; j < ahead; ++j)
        if (j < nh) issue(j);
    for (int h = 0; h < nh; ++h) {
        // younger slots of this wavefront's ring that exist: they stay in flight across the wait
        const int keep = min(ahead - 1, nh - 1 - h);
        m3_wait_vm(per * keep);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (h + ahead < nh) issue(h + ahead);
        if (needed) {
            const double *ts = ringT + (h % RT) * M3_TSLOT + (16 * wave + rc) * M3_CH;
            const double *vs = ringV + (h % RV) * VSLOT + rc * M3_CH;
            mstep_kstep<G>(ts, vs, offd, acc);
        }
    }
}

__global__ __launch_bounds__(256, M3_WPC) void k3_mstep(MSTEP_PARAMS(tiles_max), int jobs_per_pass, unsigned long long *__restrict__ dbg) {
    // all LDS of the kernel is one dynamic array (a second __shared__ object beside an LDS-DMA target can make the
    // compiler drain the vector-memory counter before LDS reads: cdna_hip_programming.md section 5)
    extern __shared__ __attribute__((aligned(16))) double m3_lds[];
    double *area = m3_lds;                                       // the rings of the current pass (m3_stream)
    int *s_jobs = reinterpret_cast<int *>(m3_lds + M3_AREA_BYTES / 8);
    double *s_tail = reinterpret_cast<double *>(s_jobs + 64);   // per job: sum of v beyond the tile's finite extent
    int *s_misc = reinterpret_cast<int *>(s_tail + 64);          // [0..3] per-wave hit counts, 5 nlo, 6 nhi, 7 need, 8 first
    unsigned long long *s_by = reinterpret_cast<unsigned long long *>(s_misc + 16);
    // after the stream of a pass the ring area is free: the cross-wave arg-max exchange lives there
    double *s_ps = area;                                        // [4][MT_MAXJ]
    int *s_pr = reinterpret_cast<int *>(area + 4 * MT_MAXJ);    // [4][MT_MAXJ]
    const unsigned lds_area = (unsigned)(size_t)(__attribute__((address_space(3))) double *)area;

    int ul, t;
    if (!mstep_block(blockIdx.x, n_utr, tiles_max, ul, t)) return;
    const int u = active[ul];
    const UtrDesc d = descs[u];
    const int B = P.B, Np = d.Np;
    const int nrows = d.T * B, row0 = t * MT_ROWS;
    if (row0 >= nrows) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double *Mu = M + (size_t)d.m_off;
    const int64_t jlo = ujob_off[u], jhi = ujob_off[u + 1];
    // There is no LDS for a tile's whole job list beside the rings: a scan stores the hits with ordinals
    // [base, base + jobs_per_pass) straight into s_jobs and returns the total; tiles with more jobs than one pass
    // holds (rare) scan again per pass.
    auto collect = [&](int base) -> int {
        return mstep_collect(ujob_list, jlo, jhi, rd_m, rd_lo, rd_hi, row0, tid, lane, wave, s_misc, [&](int off, int j) {
            if (off >= base && off < base + jobs_per_pass) s_jobs[off - base] = j;
        });
    };
    const int base0 = (int)blockIdx.y * jobs_per_pass;
    const int total = min(collect(base0), 1024);
    if (dbg && tid == 0 && blockIdx.y == 0) mstep_debug_tile(dbg, total);
    if (total <= base0) return;
    if (tid == 0) s_by[0] = s_by[1] = s_by[2] = 0ull;

    const int l8 = lane >> 3, u8 = lane & 7;
    for (int base = base0; base < total; base += jobs_per_pass * (int)gridDim.y) {
        const int cnt = min(jobs_per_pass, total - base);
        const int G = (cnt + 15) >> 4;
        if (base != base0) collect(base);      // (ends with a barrier: the previous pass's reads of s_jobs and of the exchange area are done)
        if (wave == 0) {
            MstepWin w;
            if (lane < cnt) {
                const int j = s_jobs[lane];
                w = mstep_window_of_job(rd_lo[j], rd_hi[j], rd_n0[j], rd_n1[j], row0, t);
            }
            w = mstep_window_reduce(w);
            if (lane == 0) {
                s_misc[7] = w.mk;
                s_misc[5] = w.nlo;
                s_misc[6] = w.nhi;
                s_misc[8] = w.first;
            }
        }
        __syncthreads();
        // wave-uniform by construction; readfirstlane tells the compiler so (scalar loop control, scalar DMA bases)
        const int need = __builtin_amdgcn_readfirstlane(s_misc[7]);
        const int n_ext = __builtin_amdgcn_readfirstlane(tile_nend[d.tile_off + t]);
        const MstepSpan sp = mstep_span(__builtin_amdgcn_readfirstlane(s_misc[5]), __builtin_amdgcn_readfirstlane(s_misc[6]), Np, n_ext);
        if (tid == 0 && sp.nh > 0) mstep_tally(s_by, need, nrows, row0, sp.nh, cnt, s_misc[8]);
        for (int sj = tid; sj < cnt; sj += 256) {
            const int j = s_jobs[sj];
            s_tail[sj] = Vsuf[mstep_tail_index(voff[j], j, n_ext)];
        }
        if (dbg && wave == 0) {   // how much of the MFMA work lies outside the jobs' own supports (SCAPE_HIP_DEBUG)
            int own = 0, hi_j = 0;
            if (lane < cnt) {
                const int j = s_jobs[lane];
                hi_j = max(0, min(rd_n1[j], sp.n_hi) - sp.n_lo);
                own = (max(0, min(rd_n1[j], sp.n_hi) - max(rd_n0[j] & ~15, sp.n_lo)) + 15) >> 4;
            }
            // groups of 16 after sorting by support end: every group runs to its largest end (bitonic-free: rank by counting)
            int rank = 0;
            for (int o = 0; o < 64; ++o) {
                const int other = __shfl(hi_j, o, 64);
                rank += (o < cnt) && (other > hi_j || (other == hi_j && o < lane));
            }
            int grp_sum = 0;
            for (int g = 0; g < G; ++g) {          // the largest end in sorted group g is the element of rank 16 g
                const unsigned long long m = __ballot(lane < cnt && rank == 16 * g);
                const int src = m ? __ffsll((long long)m) - 1 : 0;
                grp_sum += 16 * ((__shfl(hi_j, src, 64) + 15) >> 4);
            }
            for (int o = 32; o > 0; o >>= 1) own += __shfl_xor(own, o, 64);
            if (lane == 0) {
                atomicAdd(&dbg[16], (unsigned long long)own);
                atomicAdd(&dbg[17], (unsigned long long)cnt * sp.nh);
                atomicAdd(&dbg[18], (unsigned long long)16 * G * sp.nh);
                atomicAdd(&dbg[19], (unsigned long long)grp_sum);
            }
        }
        // per-lane DMA source offsets of this pass (bytes, relative to the uniform bases).  Rows beyond the tensor
        // and job slots beyond cnt fetch a valid neighbour instead: their products are never looked at.  Tile pieces of
        // 16-row groups that no job's window touches are not fetched at all.
        const bool needed = (need >> wave) & 1;
        unsigned offs[8], pieces = 0;
        int np_w = 0;
        if (wave < 3) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int pc = 3 * wave + i;                 // tile piece: rows 8 pc .. 8 pc + 7
                if (pc < 8 && ((need >> (pc >> 1)) & 1)) {
                    const int r = 8 * pc + l8;
                    const int rr = min(row0 + r, nrows - 1) - row0;
                    const unsigned o = (unsigned)(((size_t)rr * Np + m3_src_unit(r, u8)) * 8);
                    // compact the needed pieces to the front (np_w is wave-uniform: `need` is)
                    if (np_w == 0) offs[0] = o; else if (np_w == 1) offs[1] = o; else offs[2] = o;
                    pieces |= (unsigned)pc << (4 * np_w);
                    ++np_w;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int js = 8 * i + l8;
                const int j = s_jobs[min(js, cnt - 1)];
                offs[i] = (unsigned)((voff[j] + m3_src_unit(js, u8)) * 8);
            }
        }
        const double *tb0 = m3_uniform_ptr(Mu + (size_t)row0 * Np + sp.n_lo);
        const double *vb0 = m3_uniform_ptr(V + sp.n_lo);
        __syncthreads();   // s_tail visible
        v4f64 acc[MT_MAXJ / 16];
#pragma unroll
        for (int g = 0; g < MT_MAXJ / 16; ++g) acc[g] = (v4f64){0.0, 0.0, 0.0, 0.0};
#ifdef M3_NOSTREAM   // tools-only timing build: the per-tile set-up and arg-max epilogue without the stream (results are wrong)
        if (sp.nh < 0)
#endif
        switch (G) {
            case 1: m3_stream<1>(tb0, vb0, lds_area, area, sp.nh, wave, lane, needed, offs, np_w, pieces, acc); break;
            case 2: m3_stream<2>(tb0, vb0, lds_area, area, sp.nh, wave, lane, needed, offs, np_w, pieces, acc); break;
            case 3: m3_stream<3>(tb0, vb0, lds_area, area, sp.nh, wave, lane, needed, offs, np_w, pieces, acc); break;
            default: m3_stream<4>(tb0, vb0, lds_area, area, sp.nh, wave, lane, needed, offs, np_w, pieces, acc); break;
        }
        // the last fragment reads of the rings are done in every wavefront before the exchange area reuses them
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
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
                    b = mstep_best_of_rows(b, acc[g], c0, lo, hi, row0 + 16 * wave + kq, nrows);
                }
                b = mstep_merge_lanes(b);
                if (kq == 0 && slot_j < cnt) {
                    s_ps[wave * MT_MAXJ + slot_j] = b.score;
                    s_pr[wave * MT_MAXJ + slot_j] = b.row;
                }
            }
        }
        __syncthreads();
        for (int sj = tid; sj < cnt; sj += 256) {
            const MstepBest b = mstep_merge_waves(s_ps, s_pr, MT_MAXJ, sj);
            const int j = s_jobs[sj];
            pt_score[ptoff[j] + t] = b.score;
            pt_row[ptoff[j] + t] = mstep_row_or_fallback(b.row, rd_lo[j], row0);
        }
    }
    if (tid == 0) mstep_tally_flush(counters, s_by);
}
