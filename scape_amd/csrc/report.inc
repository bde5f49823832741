// report.inc - the two reporting stages after merge_pa (included at the end of scape_hip.hip).
//
//   ex_pa_cnt_mat   reference utils.py:438-553: per record, a pivot of (label < K) x barcode read counts, padded to every
//                   barcode of barcode_index.csv and written as a dense, fully quoted CSV row per label.
//   cal_exp_pa_len  reference utils.py:319-427 / apa_core.py:1038-1063: per record and cell cluster, the label histogram
//                   that exp_pa_len turns into an expected pA length.
//
// The device does the per-read and the per-output-byte work, all of it in exact integers:
//   k_rep_count     (record, label, barcode column) counts by 32-bit atomics, one workgroup per record
//   k_rep_complete  per-record row totals and the pivot-complete flag (every barcode that occurs in the record has a read in
//                   every row of it: pandas then keeps the pivot int64 and prints "2", otherwise float64 and "2.0")
//   k_rep_rowlen / k_rep_scan / k_rep_render
//                   byte length of every CSV row, their scan, and the row text itself (the host supplies each row's quoted
//                   pa_info prefix); rows are rendered in blocks into one of two buffers so the host compresses block b
//                   while the device renders block b + 1
//   k_rep_mtx_rowlen / k_rep_scan / k_rep_mtx_render
//                   the same rows as Matrix Market coordinate entries ("<row> <col> <count>\n", nonzero counts only,
//                   1-based): per row its entries and bytes, their scans, and the entries, through the same two slots
//   k_rep_present / k_rep_groups / k_rep_hist
//                   per record, the bitmap of cluster codes present, its compaction to the record's groups and the
//                   (group, label) histogram; labels >= K share the last slot (they decide whether a group exists and
//                   whether it has reads, never the weights)
//   k_rep_segsum    ex_pa_pseudobulk: per count row, the sum and the number of nonzero counts of every column segment
//                   (the host permutes the columns so that each pseudo-bulk sample is one contiguous segment); one wave
//                   per segment, no atomics
//   k_rep_perm_mask / k_rep_perm_rowstat / k_rep_perm_fill / k_rep_perm_test
//                   diff_pa: the membership bits of hashed label permutations (radix select of the n1-th smallest
//                   64-bit key, one workgroup per permutation), the nonzeros (position, count) of the kept count rows,
//                   and the permutation test itself (one lane per permutation, exceedance counts per site and record);
//                   section "permutation test" at the end of this file
//   k_rep_perm_mask_strata
//                   the same membership bits for labellings permuted within strata only (--strata_file): per
//                   permutation and stratum the m1[s]-th smallest key of the stratum's cells, by one wave for a stratum
//                   of up to 256 cells and by the workgroup's radix select for a larger one, one launch for all of them
//   k_rep_perm_labels / k_rep_groups_rowstat / k_rep_groups_obs / k_rep_perm_groups
//                   diff_pa_groups: the omnibus form of diff_pa for G = 2..64 populations.  One byte per (position,
//                   permutation) names the group (radix select of the G - 1 cut keys, one workgroup per
//                   permutation), and the test accumulates G sums per row and permutation in LDS; section
//                   "G-way labellings" at the end of this file
//   k_rep_perm_len  diff_pa_len: the same walk for the record's mean pA position in the two populations (one lane per
//                   permutation, two f64 sums and two integer sums per lane, exceedance counts per record)
// Cluster names, their order and the floating-point finish of exp_pa_len stay on the host (scape_amd/report.py).

#define REP_THREADS 256
#define REP_WAVES (REP_THREADS / 64)
#define REP_SCAN_THREADS 1024
#define REP_ZERO_FIELD 6   // ,"0.0"

struct ReportState {
    // counts of the last scape_hip_report_counts call
    DevBuf r_lab, r_cb, r_off, r_K, r_rowbase, r_map, r_cnt, r_tot, r_cflag, r_err;
    int32_t n_cols = 0;
    int64_t n_cnt_rows = 0;
    // histograms of the last scape_hip_report_hist call
    DevBuf h_bits, h_wpre, h_nloc, h_goff, h_hoff, h_codes, h_hist;
    std::vector<int64_t> goff, hoff;   // host side of h_goff / h_hoff: alive until the queued copies have run
    int64_t h_groups = 0, h_hist_n = 0;
    // segment sums of the last scape_hip_report_group_sums call
    DevBuf g_rows, g_off, g_sum, g_nz;
    // diff_pa: membership bits of the last scape_hip_report_perm_masks call ([column word][permutation]) and the
    // buffers of scape_hip_report_perm_test
    DevBuf m_bits, p_rows, p_roff, p_nnz, p_noff, p_nz, p_t, p_a0, p_recs, p_site, p_gene, p_stat0;
    DevBuf l_w, l_tol;                 // diff_pa_len: row weights and record tolerances of scape_hip_report_perm_len
    int32_t m_n1 = 0, m_n2 = 0, m_count = 0;
    // stratified masks: (a1, m1, a2, m2) per stratum, the strata in work order, the stratum of every position and the
    // exclusive key bound per (permutation, stratum)
    DevBuf m_desc, m_order, m_strat, m_bound;
    // diff_pa_groups: the group of every (position, permutation) of the last scape_hip_report_perm_labels call
    // ([position][permutation], one byte each), the ranks of its cut keys, and the buffers of
    // scape_hip_report_perm_groups that scape_hip_report_perm_test has no counterpart of
    DevBuf q_lab, q_cut, q_seg, q_a0, q_s0, q_share;
    std::vector<int32_t> q_sizes;      // cells per group of the last labels call
    int32_t q_n = 0, q_count = 0;
    // render slots
    DevBuf s_rows[2], s_int[2], s_poff[2], s_pre[2], s_len[2], s_roff[2], s_out[2];
    DevBuf s_nnz[2], s_noff[2];        // Matrix Market blocks: entries per row and their scan
    void *host_out[2] = {nullptr, nullptr};
    size_t host_cap[2] = {0, 0};
    int64_t slot_bytes[2] = {0, 0};
    hipEvent_t done[2] = {nullptr, nullptr};
    bool pending[2] = {false, false};
};

static void report_release(scape_hip_ctx *c) {
    ReportState *s = c->rep;
    if (!s) return;
    for (int k = 0; k < 2; ++k) {
        if (s->done[k]) (void)hipEventSynchronize(s->done[k]);
        if (s->done[k]) (void)hipEventDestroy(s->done[k]);
        if (s->host_out[k]) (void)hipHostFree(s->host_out[k]);
    }
    DevBuf *all[] = {&s->r_lab, &s->r_cb, &s->r_off, &s->r_K, &s->r_rowbase, &s->r_map, &s->r_cnt, &s->r_tot,
                     &s->r_cflag, &s->r_err, &s->h_bits, &s->h_wpre, &s->h_nloc, &s->h_goff, &s->h_hoff, &s->h_codes,
                     &s->h_hist, &s->s_rows[0], &s->s_rows[1], &s->s_int[0], &s->s_int[1], &s->s_poff[0],
                     &s->s_poff[1], &s->s_pre[0], &s->s_pre[1], &s->s_len[0], &s->s_len[1], &s->s_roff[0],
                     &s->s_roff[1], &s->s_out[0], &s->s_out[1], &s->s_nnz[0], &s->s_nnz[1], &s->s_noff[0],
                     &s->s_noff[1], &s->g_rows, &s->g_off, &s->g_sum, &s->g_nz, &s->m_bits, &s->p_rows,
                     &s->p_roff, &s->p_nnz, &s->p_noff, &s->p_nz, &s->p_t, &s->p_a0, &s->p_recs, &s->p_site, &s->p_gene,
                     &s->p_stat0, &s->l_w, &s->l_tol, &s->m_desc, &s->m_order, &s->m_strat, &s->m_bound,
                     &s->q_lab, &s->q_cut, &s->q_seg, &s->q_a0, &s->q_s0, &s->q_share};
    for (DevBuf *b : all) b->release();
    delete s;
    c->rep = nullptr;
}

static ReportState *report_state(scape_hip_ctx *c) {
    if (!c->rep) c->rep = new ReportState();
    return c->rep;
}

// ---- block helpers (REP_THREADS or REP_SCAN_THREADS threads, wave64) ----------------------------------------------
template <typename T, int NW>
__device__ __forceinline__ T rep_block_sum(T v, T *lds) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if (lane == 0) lds[w] = v;
    __syncthreads();
    T t = 0;
    for (int k = 0; k < NW; ++k) t += lds[k];
    return t;
}

// exclusive scan over the block; *total gets the block's sum
template <typename T, int NW>
__device__ __forceinline__ T rep_block_excl(T v, T *lds, T *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    __syncthreads();
    if (lane == 63) lds[w] = x;
    __syncthreads();
    T before = 0, all = 0;
    for (int k = 0; k < NW; ++k) {
        const T s = lds[k];
        if (k < w) before += s;
        all += s;
    }
    *total = all;
    return before + x - v;
}

__device__ __forceinline__ int rep_digits(uint32_t v) {
    int n = 1;
    while (v >= 10) {
        v /= 10;
        ++n;
    }
    return n;
}

__device__ __forceinline__ int rep_digits64(uint64_t v) {
    int n = 1;
    while (v >= 10) {
        v /= 10;
        ++n;
    }
    return n;
}

// bytes a count adds over the constant zero field "0.0": "7" -> -2, "7.0" -> 0, "12" -> -1, "12.0" -> +1
__device__ __forceinline__ int rep_extra(int v, int is_int) {
    return v == 0 ? 0 : rep_digits((uint32_t)v) + (is_int ? -3 : -1);
}

// ---- counts ---------------------------------------------------------------------------------------------------------
// one workgroup per record; err[0] = first read (label < K) whose barcode id has no column, err[1] = first read with a
// negative label (both start at INT64_MAX)
__global__ __launch_bounds__(REP_THREADS) void k_rep_count(const int64_t *__restrict__ read_off,
                                                           const int32_t *__restrict__ Ks,
                                                           const int64_t *__restrict__ rowbase,
                                                           const int64_t *__restrict__ label,
                                                           const int64_t *__restrict__ cb, int64_t id_min,
                                                           int64_t id_span, const int32_t *__restrict__ id2col,
                                                           int32_t n_cols, int32_t *__restrict__ cnt,
                                                           unsigned long long *__restrict__ err) {
    const int r = blockIdx.x;
    const int64_t K = Ks[r], row0 = rowbase[r];
    for (int64_t i = read_off[r] + threadIdx.x; i < read_off[r + 1]; i += REP_THREADS) {
        const int64_t lab = label[i];
        if (lab < 0) {
            atomicMin(&err[1], (unsigned long long)i);
            continue;
        }
        if (lab >= K) continue;
        const int64_t d = cb[i] - id_min;
        const int col = (d >= 0 && d < id_span) ? id2col[d] : -1;
        if (col < 0) {
            atomicMin(&err[0], (unsigned long long)i);
            continue;
        }
        atomicAdd(&cnt[(row0 + lab) * n_cols + col], 1);
    }
}

// one workgroup per record: row totals tot[row0 + l], and complete[r] = (sum over columns of the rows a column has reads
// in == columns with reads x rows with reads)
__global__ __launch_bounds__(REP_THREADS) void k_rep_complete(const int32_t *__restrict__ Ks,
                                                              const int64_t *__restrict__ rowbase, int32_t n_cols,
                                                              const int32_t *__restrict__ cnt,
                                                              int64_t *__restrict__ tot, int8_t *__restrict__ complete) {
    __shared__ long long lds[REP_WAVES];
    const int r = blockIdx.x;
    const int K = Ks[r];
    const int64_t row0 = rowbase[r];
    long long n_rows = 0;
    for (int l = 0; l < K; ++l) {
        const int32_t *row = cnt + (row0 + l) * n_cols;
        long long s = 0;
        for (int c = threadIdx.x; c < n_cols; c += REP_THREADS) s += row[c];
        s = rep_block_sum<long long, REP_WAVES>(s, lds);
        if (threadIdx.x == 0) tot[row0 + l] = s;
        n_rows += s > 0;
    }
    long long nz = 0, occ = 0;
    for (int c = threadIdx.x; c < n_cols; c += REP_THREADS) {
        int k = 0;
        for (int l = 0; l < K; ++l) k += cnt[(row0 + l) * n_cols + c] > 0;
        nz += k;
        occ += k > 0;
    }
    nz = rep_block_sum<long long, REP_WAVES>(nz, lds);
    occ = rep_block_sum<long long, REP_WAVES>(occ, lds);
    if (threadIdx.x == 0) complete[r] = nz == occ * n_rows;
}

// ---- rendering ------------------------------------------------------------------------------------------------------
// row i of a block: count row rows[i] of the last counts call, integer form is_int[i], prefix bytes [poff[i], poff[i+1])
__global__ __launch_bounds__(REP_THREADS) void k_rep_rowlen(const int64_t *__restrict__ rows,
                                                            const int8_t *__restrict__ is_int,
                                                            const int64_t *__restrict__ poff, int32_t n_cols,
                                                            const int32_t *__restrict__ cnt,
                                                            int64_t *__restrict__ rlen) {
    __shared__ long long lds[REP_WAVES];
    const int i = blockIdx.x;
    const int32_t *row = cnt + rows[i] * n_cols;
    const int ii = is_int[i];
    long long e = 0;
    for (int c = threadIdx.x; c < n_cols; c += REP_THREADS) e += rep_extra(row[c], ii);
    e = rep_block_sum<long long, REP_WAVES>(e, lds);
    if (threadIdx.x == 0) rlen[i] = (poff[i + 1] - poff[i]) + (long long)REP_ZERO_FIELD * n_cols + e + 1;
}

// one workgroup: roff[i] = sum of rlen[0..i), roff[n] = the block's bytes
__global__ __launch_bounds__(REP_SCAN_THREADS) void k_rep_scan(const int64_t *__restrict__ rlen, int32_t n,
                                                               int64_t *__restrict__ roff) {
    __shared__ long long lds[REP_SCAN_THREADS / 64];
    long long carry = 0;
    for (int base = 0; base < n; base += REP_SCAN_THREADS) {
        const int i = base + threadIdx.x;
        const long long v = i < n ? rlen[i] : 0;
        long long tot;
        const long long ex = rep_block_excl<long long, REP_SCAN_THREADS / 64>(v, lds, &tot);
        if (i < n) roff[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) roff[n] = carry;
}

// one workgroup per row: the prefix, then 256 columns per step - each lane's field position is the tile's running
// offset plus the exclusive scan of the field lengths - then the newline
__global__ __launch_bounds__(REP_THREADS) void k_rep_render(const int64_t *__restrict__ rows,
                                                            const int8_t *__restrict__ is_int,
                                                            const int64_t *__restrict__ poff,
                                                            const char *__restrict__ pre, int32_t n_cols,
                                                            const int32_t *__restrict__ cnt,
                                                            const int64_t *__restrict__ roff, char *__restrict__ out) {
    __shared__ int lds[REP_WAVES];
    const int i = blockIdx.x;
    const int32_t *row = cnt + rows[i] * n_cols;
    const int ii = is_int[i];
    char *dst = out + roff[i];
    const int64_t p0 = poff[i], plen = poff[i + 1] - p0;
    for (int64_t k = threadIdx.x; k < plen; k += REP_THREADS) dst[k] = pre[p0 + k];
    int64_t pos = plen;
    for (int base = 0; base < n_cols; base += REP_THREADS) {
        const int c = base + threadIdx.x;
        const int v = c < n_cols ? row[c] : 0;
        const int flen = c < n_cols ? REP_ZERO_FIELD + rep_extra(v, ii) : 0;
        int tile;
        const int ex = rep_block_excl<int, REP_WAVES>(flen, lds, &tile);
        if (c < n_cols) {
            char *f = dst + pos + ex;
            f[0] = ',';
            f[1] = '"';
            if (v == 0) {
                f[2] = '0';
                f[3] = '.';
                f[4] = '0';
                f[5] = '"';
            } else {
                const int nd = rep_digits((uint32_t)v);
                uint32_t x = (uint32_t)v;
                for (int d = nd - 1; d >= 0; --d) {
                    f[2 + d] = (char)('0' + x % 10);
                    x /= 10;
                }
                int e = 2 + nd;
                if (!ii) {
                    f[e++] = '.';
                    f[e++] = '0';
                }
                f[e] = '"';
            }
        }
        pos += tile;
    }
    if (threadIdx.x == 0) dst[pos] = '\n';
}

// ---- Matrix Market rendering ----------------------------------------------------------------------------------------
// row i of a block: count row rows[i] of the last counts call, number row_no0 + i of the file; its entries are
// "<row number> <column + 1> <count>\n" for the nonzero columns, ascending.  rnnz[i] = entries, rlen[i] = bytes
__global__ __launch_bounds__(REP_THREADS) void k_rep_mtx_rowlen(const int64_t *__restrict__ rows, int64_t row_no0,
                                                                int32_t n_cols, const int32_t *__restrict__ cnt,
                                                                int64_t *__restrict__ rlen,
                                                                int64_t *__restrict__ rnnz) {
    __shared__ long long lds[REP_WAVES];
    const int i = blockIdx.x;
    const int32_t *row = cnt + rows[i] * n_cols;
    long long n = 0, e = 0;
    for (int c = threadIdx.x; c < n_cols; c += REP_THREADS) {
        const int v = row[c];
        if (v) {
            ++n;
            e += rep_digits((uint32_t)c + 1) + rep_digits((uint32_t)v);
        }
    }
    n = rep_block_sum<long long, REP_WAVES>(n, lds);
    e = rep_block_sum<long long, REP_WAVES>(e, lds);
    if (threadIdx.x == 0) {
        rnnz[i] = n;
        rlen[i] = e + n * (rep_digits64((uint64_t)(row_no0 + i)) + 3);   // two spaces and the newline
    }
}

// one workgroup per row, 256 columns per step: each lane's entry position is the tile's running offset plus the
// exclusive scan of the entry lengths (0 for a zero count); the row number is formatted once, into LDS
__global__ __launch_bounds__(REP_THREADS) void k_rep_mtx_render(const int64_t *__restrict__ rows, int64_t row_no0,
                                                                int32_t n_cols, const int32_t *__restrict__ cnt,
                                                                const int64_t *__restrict__ roff,
                                                                char *__restrict__ out) {
    __shared__ int lds[REP_WAVES];
    __shared__ char row_txt[20];
    const int i = blockIdx.x;
    const int32_t *row = cnt + rows[i] * n_cols;
    const uint64_t row_no = (uint64_t)(row_no0 + i);
    const int rd = rep_digits64(row_no);
    if (threadIdx.x == 0) {
        uint64_t x = row_no;
        for (int d = rd - 1; d >= 0; --d) {
            row_txt[d] = (char)('0' + x % 10);
            x /= 10;
        }
    }
    __syncthreads();
    char *dst = out + roff[i];
    int64_t pos = 0;
    for (int base = 0; base < n_cols; base += REP_THREADS) {
        const int c = base + threadIdx.x;
        const int v = c < n_cols ? row[c] : 0;
        const int cd = v ? rep_digits((uint32_t)c + 1) : 0;
        const int vd = v ? rep_digits((uint32_t)v) : 0;
        const int elen = v ? rd + cd + vd + 3 : 0;
        int tile;
        const int ex = rep_block_excl<int, REP_WAVES>(elen, lds, &tile);
        if (v) {
            char *f = dst + pos + ex;
            for (int d = 0; d < rd; ++d) f[d] = row_txt[d];
            f[rd] = ' ';
            f += rd + 1;
            uint32_t x = (uint32_t)c + 1;
            for (int d = cd - 1; d >= 0; --d) {
                f[d] = (char)('0' + x % 10);
                x /= 10;
            }
            f[cd] = ' ';
            f += cd + 1;
            x = (uint32_t)v;
            for (int d = vd - 1; d >= 0; --d) {
                f[d] = (char)('0' + x % 10);
                x /= 10;
            }
            f[vd] = '\n';
        }
        pos += tile;
    }
}

// ---- segment sums (pseudo-bulk) ---------------------------------------------------------------------------------------
// one workgroup per row i (count row rows[i] of the last counts call); segment s is the columns [seg_off[s], seg_off[s+1]).
// Wave w takes segments w, w + REP_WAVES, ...: its lanes stride the segment, then the wave adds up.  sum / nz are
// [row][segment]; a row's sum fits 32 bits because a record holds at most INT32_MAX reads
__global__ __launch_bounds__(REP_THREADS) void k_rep_segsum(const int64_t *__restrict__ rows, int32_t n_cols,
                                                            const int32_t *__restrict__ cnt, int32_t n_seg,
                                                            const int32_t *__restrict__ seg_off,
                                                            int32_t *__restrict__ sum, int32_t *__restrict__ nz) {
    const int i = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int32_t *row = cnt + rows[i] * n_cols;
    int32_t *so = sum + (int64_t)i * n_seg, *zo = nz + (int64_t)i * n_seg;
    for (int s = w; s < n_seg; s += REP_WAVES) {
        const int a = seg_off[s], b = seg_off[s + 1];
        int t = 0, z = 0;
#pragma unroll 4
        for (int c = a + lane; c < b; c += 64) {
            const int v = row[c];
            t += v;
            z += v > 0;
        }
        for (int o = 32; o > 0; o >>= 1) {
            t += __shfl_xor(t, o, 64);
            z += __shfl_xor(z, o, 64);
        }
        if (lane == 0) {
            so[s] = t;
            zo[s] = z;
        }
    }
}

// ---- cluster histograms ---------------------------------------------------------------------------------------------
// one workgroup per record: bit `code` of the record's bitmap for every read; id2code == nullptr: one group (code 0).
// err[0] = first read whose barcode id has no code, err[1] = first read with a negative label
__global__ __launch_bounds__(REP_THREADS) void k_rep_present(const int64_t *__restrict__ read_off,
                                                             const int64_t *__restrict__ label,
                                                             const int64_t *__restrict__ cb, int64_t id_min,
                                                             int64_t id_span, const int32_t *__restrict__ id2code,
                                                             int32_t n_words, uint32_t *__restrict__ bits,
                                                             unsigned long long *__restrict__ err) {
    const int r = blockIdx.x;
    uint32_t *b = bits + (int64_t)r * n_words;
    for (int64_t i = read_off[r] + threadIdx.x; i < read_off[r + 1]; i += REP_THREADS) {
        if (label[i] < 0) atomicMin(&err[1], (unsigned long long)i);
        int code = 0;
        if (id2code) {
            const int64_t d = cb[i] - id_min;
            code = (d >= 0 && d < id_span) ? id2code[d] : -1;
            if (code < 0) {
                atomicMin(&err[0], (unsigned long long)i);
                continue;
            }
        }
        atomicOr(&b[code >> 5], 1u << (code & 31));
    }
}

// one workgroup per record: wpre[w] = set bits of the record's words before w, nloc[r] = groups of the record
__global__ __launch_bounds__(REP_THREADS) void k_rep_groups(int32_t n_words, const uint32_t *__restrict__ bits,
                                                            int32_t *__restrict__ wpre, int64_t *__restrict__ nloc) {
    __shared__ int lds[REP_WAVES];
    const int r = blockIdx.x;
    const uint32_t *b = bits + (int64_t)r * n_words;
    int32_t *p = wpre + (int64_t)r * n_words;
    int carry = 0;
    for (int base = 0; base < n_words; base += REP_THREADS) {
        const int w = base + threadIdx.x;
        const int v = w < n_words ? __popc(b[w]) : 0;
        int tile;
        const int ex = rep_block_excl<int, REP_WAVES>(v, lds, &tile);
        if (w < n_words) p[w] = carry + ex;
        carry += tile;
    }
    if (threadIdx.x == 0) nloc[r] = carry;
}

// one workgroup per record: the record's group codes in ascending code order, and the (group, min(label, K)) counts
__global__ __launch_bounds__(REP_THREADS) void k_rep_hist(const int64_t *__restrict__ read_off,
                                                          const int32_t *__restrict__ Ks,
                                                          const int64_t *__restrict__ label,
                                                          const int64_t *__restrict__ cb, int64_t id_min,
                                                          const int32_t *__restrict__ id2code, int32_t n_words,
                                                          const uint32_t *__restrict__ bits,
                                                          const int32_t *__restrict__ wpre,
                                                          const int64_t *__restrict__ goff,
                                                          const int64_t *__restrict__ hoff,
                                                          int32_t *__restrict__ codes, int32_t *__restrict__ hist) {
    const int r = blockIdx.x;
    const uint32_t *b = bits + (int64_t)r * n_words;
    const int32_t *p = wpre + (int64_t)r * n_words;
    for (int w = threadIdx.x; w < n_words; w += REP_THREADS) {
        uint32_t m = b[w];
        int k = p[w];
        while (m) {
            const int j = __ffs(m) - 1;
            codes[goff[r] + k++] = w * 32 + j;
            m &= m - 1;
        }
    }
    const int64_t K = Ks[r];
    int32_t *h = hist + hoff[r];
    for (int64_t i = read_off[r] + threadIdx.x; i < read_off[r + 1]; i += REP_THREADS) {
        const int64_t lab = label[i];
        if (lab < 0) continue;
        int code = 0;
        if (id2code) {
            code = id2code[cb[i] - id_min];   // k_rep_present checked every id
        }
        const int w = code >> 5;
        const int g = p[w] + __popc(b[w] & ((1u << (code & 31)) - 1u));
        atomicAdd(&h[(int64_t)g * (K + 1) + (lab < K ? lab : K)], 1);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
static int rep_upload_reads(scape_hip_ctx *c, ReportState *s, int32_t n_rec, const int64_t *read_off,
                            const int32_t *K, const int64_t *label, const int64_t *cb_id) {
    if (n_rec <= 0) return fail("n_rec must be positive");
    if (!read_off || !K || !label || !cb_id) return fail("NULL array");
    const int64_t n = read_off[n_rec];
    if (read_off[0] != 0 || n < 0) return fail("read_off must start at 0 and end at the read count");
    for (int r = 0; r < n_rec; ++r) {
        if (read_off[r + 1] < read_off[r]) return fail("read_off must be non-decreasing");
        if (read_off[r + 1] - read_off[r] > INT32_MAX) return fail("a record has more reads than 32-bit counts hold");
        if (K[r] < 1) return fail("K must be positive");
    }
    if (s->r_lab.ensure(n * 8) || s->r_cb.ensure(n * 8) || s->r_off.ensure((n_rec + 1) * 8) || s->r_K.ensure(n_rec * 4) ||
        s->r_err.ensure(16))
        return 1;
    if (n) {
        HIPCHK(hipMemcpyAsync(s->r_lab.p, label, n * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(s->r_cb.p, cb_id, n * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipMemcpyAsync(s->r_off.p, read_off, (n_rec + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->r_K.p, K, n_rec * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(s->r_err.p, 0xff, 16, c->stream));
    return 0;
}

static int rep_upload_map(scape_hip_ctx *c, ReportState *s, int64_t id_span, const int32_t *id2x) {
    if (id_span < 0 || (id_span > 0 && !id2x)) return fail("bad barcode id map");
    if (s->r_map.ensure(std::max<int64_t>(id_span, 1) * 4)) return 1;
    if (id_span) HIPCHK(hipMemcpyAsync(s->r_map.p, id2x, id_span * 4, hipMemcpyHostToDevice, c->stream));
    return 0;
}

// a render slot's device text buffer, pinned host buffer and event, for a block of `total` bytes
static int rep_slot_out(ReportState *s, int32_t slot, int64_t total) {
    if (s->s_out[slot].ensure(total)) return 1;
    if (s->host_cap[slot] < (size_t)total) {
        if (s->host_out[slot]) HIPCHK(hipHostFree(s->host_out[slot]));
        s->host_out[slot] = nullptr;
        s->host_cap[slot] = 0;
        const size_t want = (size_t)total + (size_t)total / 8;
        HIPCHK(hipHostMalloc(&s->host_out[slot], want, hipHostMallocDefault));
        s->host_cap[slot] = want;
    }
    if (!s->done[slot]) HIPCHK(hipEventCreateWithFlags(&s->done[slot], hipEventDisableTiming));
    return 0;
}

// queue the copy of a rendered block into the slot's pinned host buffer (scape_hip_report_fetch waits for it)
static int rep_slot_queue(scape_hip_ctx *c, ReportState *s, int32_t slot, int64_t total) {
    HIPCHK(hipMemcpyAsync(s->host_out[slot], s->s_out[slot].p, total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(s->done[slot], c->stream));
    s->pending[slot] = true;
    s->slot_bytes[slot] = total;
    return 0;
}

static int rep_fetch_err(scape_hip_ctx *c, ReportState *s, int64_t *bad) {
    unsigned long long e[2];
    HIPCHK(hipMemcpyAsync(e, s->r_err.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 2; ++k) bad[k] = e[k] == ~0ull ? -1 : (int64_t)e[k];
    return 0;
}

extern "C" {

int scape_hip_report_counts(scape_hip_ctx *c, int32_t n_rec, const int64_t *read_off, const int32_t *K,
                            const int64_t *label, const int64_t *cb_id, int64_t id_min, int64_t id_span,
                            const int32_t *id2col, int32_t n_cols, int64_t *row_tot_out, int8_t *complete_out,
                            int64_t *bad_read_out) {
    CTX_ENTER(c);
    if (n_cols <= 0 || !row_tot_out || !complete_out || !bad_read_out) return fail("bad argument");
    ReportState *s = report_state(c);
    for (int k = 0; k < 2; ++k)          // the render slots read the counts buffer: finish them first
        if (s->pending[k]) HIPCHK(hipEventSynchronize(s->done[k]));
    if (rep_upload_reads(c, s, n_rec, read_off, K, label, cb_id) || rep_upload_map(c, s, id_span, id2col)) return 1;
    std::vector<int64_t> rowbase(n_rec);
    int64_t rows = 0;
    for (int r = 0; r < n_rec; ++r) {
        rowbase[r] = rows;
        rows += K[r];
    }
    if (s->r_rowbase.ensure(n_rec * 8) || s->r_cnt.ensure(rows * n_cols * 4) || s->r_tot.ensure(rows * 8) ||
        s->r_cflag.ensure(n_rec))
        return 1;
    HIPCHK(hipMemcpyAsync(s->r_rowbase.p, rowbase.data(), n_rec * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(s->r_cnt.p, 0, rows * n_cols * 4, c->stream));
    hipLaunchKernelGGL(k_rep_count, dim3(n_rec), dim3(REP_THREADS), 0, c->stream, s->r_off.as<int64_t>(),
                       s->r_K.as<int32_t>(), s->r_rowbase.as<int64_t>(), s->r_lab.as<int64_t>(), s->r_cb.as<int64_t>(),
                       id_min, id_span, s->r_map.as<int32_t>(), n_cols, s->r_cnt.as<int32_t>(),
                       s->r_err.as<unsigned long long>());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rep_complete, dim3(n_rec), dim3(REP_THREADS), 0, c->stream, s->r_K.as<int32_t>(),
                       s->r_rowbase.as<int64_t>(), n_cols, s->r_cnt.as<int32_t>(), s->r_tot.as<int64_t>(),
                       s->r_cflag.as<int8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(row_tot_out, s->r_tot.p, rows * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(complete_out, s->r_cflag.p, n_rec, hipMemcpyDeviceToHost, c->stream));
    if (rep_fetch_err(c, s, bad_read_out)) return 1;
    s->n_cols = n_cols;
    s->n_cnt_rows = rows;
    return 0;
}

int scape_hip_report_render(scape_hip_ctx *c, int32_t slot, int32_t n_rows, const int64_t *rows, const int8_t *is_int,
                            const int64_t *pre_off, const char *pre, int64_t *bytes_out) {
    CTX_ENTER(c);
    ReportState *s = c->rep;
    if (!s || !s->n_cnt_rows) return fail("scape_hip_report_counts has not been called");
    if (slot < 0 || slot > 1 || n_rows <= 0 || !rows || !is_int || !pre_off || !pre || !bytes_out)
        return fail("bad argument");
    for (int i = 0; i < n_rows; ++i)
        if (rows[i] < 0 || rows[i] >= s->n_cnt_rows) return fail("row index out of range");
    if (pre_off[0] != 0) return fail("pre_off must start at 0");
    for (int i = 0; i < n_rows; ++i)
        if (pre_off[i + 1] < pre_off[i]) return fail("pre_off must be non-decreasing");
    if (s->pending[slot]) {              // the host buffer of this slot is handed over again
        HIPCHK(hipEventSynchronize(s->done[slot]));
        s->pending[slot] = false;
    }
    const int64_t pre_n = pre_off[n_rows];
    if (s->s_rows[slot].ensure(n_rows * 8) || s->s_int[slot].ensure(n_rows) || s->s_poff[slot].ensure((n_rows + 1) * 8) ||
        s->s_pre[slot].ensure(std::max<int64_t>(pre_n, 1)) || s->s_len[slot].ensure(n_rows * 8) ||
        s->s_roff[slot].ensure((n_rows + 1) * 8))
        return 1;
    HIPCHK(hipMemcpyAsync(s->s_rows[slot].p, rows, n_rows * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->s_int[slot].p, is_int, n_rows, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->s_poff[slot].p, pre_off, (n_rows + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (pre_n) HIPCHK(hipMemcpyAsync(s->s_pre[slot].p, pre, pre_n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_rep_rowlen, dim3(n_rows), dim3(REP_THREADS), 0, c->stream, s->s_rows[slot].as<int64_t>(),
                       s->s_int[slot].as<int8_t>(), s->s_poff[slot].as<int64_t>(), s->n_cols, s->r_cnt.as<int32_t>(),
                       s->s_len[slot].as<int64_t>());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rep_scan, dim3(1), dim3(REP_SCAN_THREADS), 0, c->stream, s->s_len[slot].as<int64_t>(), n_rows,
                       s->s_roff[slot].as<int64_t>());
    HIPCHK(hipGetLastError());
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, s->s_roff[slot].as<int64_t>() + n_rows, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (total <= 0) return fail("empty render block");
    if (rep_slot_out(s, slot, total)) return 1;
    hipLaunchKernelGGL(k_rep_render, dim3(n_rows), dim3(REP_THREADS), 0, c->stream, s->s_rows[slot].as<int64_t>(),
                       s->s_int[slot].as<int8_t>(), s->s_poff[slot].as<int64_t>(), s->s_pre[slot].as<char>(), s->n_cols,
                       s->r_cnt.as<int32_t>(), s->s_roff[slot].as<int64_t>(), s->s_out[slot].as<char>());
    HIPCHK(hipGetLastError());
    if (rep_slot_queue(c, s, slot, total)) return 1;
    *bytes_out = total;
    return 0;
}

int scape_hip_report_render_mtx(scape_hip_ctx *c, int32_t slot, int32_t n_rows, const int64_t *rows, int64_t row_no0,
                                int64_t *bytes_out, int64_t *nnz_out) {
    CTX_ENTER(c);
    ReportState *s = c->rep;
    if (!s || !s->n_cnt_rows) return fail("scape_hip_report_counts has not been called");
    if (slot < 0 || slot > 1 || n_rows <= 0 || !rows || !bytes_out || !nnz_out) return fail("bad argument");
    if (row_no0 < 1 || row_no0 > INT64_MAX - n_rows) return fail("row_no0 out of range");
    for (int i = 0; i < n_rows; ++i)
        if (rows[i] < 0 || rows[i] >= s->n_cnt_rows) return fail("row index out of range");
    if (s->pending[slot]) {              // the host buffer of this slot is handed over again
        HIPCHK(hipEventSynchronize(s->done[slot]));
        s->pending[slot] = false;
    }
    const int64_t n = n_rows;
    if (s->s_rows[slot].ensure(n * 8) || s->s_len[slot].ensure(n * 8) || s->s_roff[slot].ensure((n + 1) * 8) ||
        s->s_nnz[slot].ensure(n * 8) || s->s_noff[slot].ensure((n + 1) * 8))
        return 1;
    HIPCHK(hipMemcpyAsync(s->s_rows[slot].p, rows, n * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_rep_mtx_rowlen, dim3(n_rows), dim3(REP_THREADS), 0, c->stream, s->s_rows[slot].as<int64_t>(),
                       row_no0, s->n_cols, s->r_cnt.as<int32_t>(), s->s_len[slot].as<int64_t>(),
                       s->s_nnz[slot].as<int64_t>());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rep_scan, dim3(1), dim3(REP_SCAN_THREADS), 0, c->stream, s->s_len[slot].as<int64_t>(), n_rows,
                       s->s_roff[slot].as<int64_t>());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rep_scan, dim3(1), dim3(REP_SCAN_THREADS), 0, c->stream, s->s_nnz[slot].as<int64_t>(), n_rows,
                       s->s_noff[slot].as<int64_t>());
    HIPCHK(hipGetLastError());
    int64_t total = 0, nnz = 0;
    HIPCHK(hipMemcpyAsync(&total, s->s_roff[slot].as<int64_t>() + n_rows, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&nnz, s->s_noff[slot].as<int64_t>() + n_rows, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (total <= 0) return fail("empty render block");
    if (rep_slot_out(s, slot, total)) return 1;
    hipLaunchKernelGGL(k_rep_mtx_render, dim3(n_rows), dim3(REP_THREADS), 0, c->stream, s->s_rows[slot].as<int64_t>(),
                       row_no0, s->n_cols, s->r_cnt.as<int32_t>(), s->s_roff[slot].as<int64_t>(),
                       s->s_out[slot].as<char>());
    HIPCHK(hipGetLastError());
    if (rep_slot_queue(c, s, slot, total)) return 1;
    *bytes_out = total;
    *nnz_out = nnz;
    return 0;
}

int scape_hip_report_group_sums(scape_hip_ctx *c, int32_t n_seg, const int32_t *seg_off, int32_t n_rows,
                                const int64_t *rows, int32_t *sum_out, int32_t *nz_out) {
    CTX_ENTER(c);
    ReportState *s = c->rep;
    if (!s || !s->n_cnt_rows) return fail("scape_hip_report_counts has not been called");
    if (n_seg <= 0 || n_rows <= 0 || !seg_off || !rows || !sum_out || !nz_out) return fail("bad argument");
    if (seg_off[0] < 0 || seg_off[n_seg] > s->n_cols) return fail("seg_off must lie within the columns");
    for (int k = 0; k < n_seg; ++k)
        if (seg_off[k + 1] < seg_off[k]) return fail("seg_off must be non-decreasing");
    for (int i = 0; i < n_rows; ++i)
        if (rows[i] < 0 || rows[i] >= s->n_cnt_rows) return fail("row index out of range");
    const int64_t n_out = (int64_t)n_rows * n_seg;
    if (s->g_rows.ensure((int64_t)n_rows * 8) || s->g_off.ensure(((int64_t)n_seg + 1) * 4) || s->g_sum.ensure(n_out * 4) ||
        s->g_nz.ensure(n_out * 4))
        return 1;
    HIPCHK(hipMemcpyAsync(s->g_rows.p, rows, (int64_t)n_rows * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->g_off.p, seg_off, ((int64_t)n_seg + 1) * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_rep_segsum, dim3(n_rows), dim3(REP_THREADS), 0, c->stream, s->g_rows.as<int64_t>(), s->n_cols,
                       s->r_cnt.as<int32_t>(), n_seg, s->g_off.as<int32_t>(), s->g_sum.as<int32_t>(),
                       s->g_nz.as<int32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sum_out, s->g_sum.p, n_out * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(nz_out, s->g_nz.p, n_out * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int scape_hip_report_fetch(scape_hip_ctx *c, int32_t slot, void **host_ptr, int64_t *bytes_out) {
    CTX_ENTER(c);
    ReportState *s = c->rep;
    if (!s || slot < 0 || slot > 1 || !host_ptr || !bytes_out) return fail("bad argument");
    if (!s->pending[slot]) return fail("nothing rendered into this slot");
    HIPCHK(hipEventSynchronize(s->done[slot]));
    s->pending[slot] = false;
    *host_ptr = s->host_out[slot];
    *bytes_out = s->slot_bytes[slot];
    return 0;
}

int scape_hip_report_hist(scape_hip_ctx *c, int32_t n_rec, const int64_t *read_off, const int32_t *K,
                          const int64_t *label, const int64_t *cb_id, int64_t id_min, int64_t id_span,
                          const int32_t *id2code, int32_t n_codes, int64_t *n_groups_out, int64_t *bad_read_out) {
    CTX_ENTER(c);
    if (n_codes <= 0 || !n_groups_out || !bad_read_out) return fail("bad argument");
    ReportState *s = report_state(c);
    if (rep_upload_reads(c, s, n_rec, read_off, K, label, cb_id)) return 1;
    if (id2code && rep_upload_map(c, s, id_span, id2code)) return 1;
    const int32_t n_words = (n_codes + 31) / 32;
    const int64_t nw = (int64_t)n_rec * n_words;
    if (s->h_bits.ensure(nw * 4) || s->h_wpre.ensure(nw * 4) || s->h_nloc.ensure(n_rec * 8)) return 1;
    HIPCHK(hipMemsetAsync(s->h_bits.p, 0, nw * 4, c->stream));
    const int32_t *map = id2code ? s->r_map.as<int32_t>() : nullptr;
    hipLaunchKernelGGL(k_rep_present, dim3(n_rec), dim3(REP_THREADS), 0, c->stream, s->r_off.as<int64_t>(),
                       s->r_lab.as<int64_t>(), s->r_cb.as<int64_t>(), id_min, id_span, map, n_words,
                       s->h_bits.as<uint32_t>(), s->r_err.as<unsigned long long>());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rep_groups, dim3(n_rec), dim3(REP_THREADS), 0, c->stream, n_words, s->h_bits.as<uint32_t>(),
                       s->h_wpre.as<int32_t>(), s->h_nloc.as<int64_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(n_groups_out, s->h_nloc.p, n_rec * 8, hipMemcpyDeviceToHost, c->stream));
    if (rep_fetch_err(c, s, bad_read_out)) return 1;
    s->h_groups = s->h_hist_n = 0;
    if (bad_read_out[0] >= 0 || bad_read_out[1] >= 0) return 0;
    std::vector<int64_t> &goff = s->goff, &hoff = s->hoff;
    goff.resize(n_rec);
    hoff.resize(n_rec);
    for (int r = 0; r < n_rec; ++r) {
        goff[r] = s->h_groups;
        hoff[r] = s->h_hist_n;
        s->h_groups += n_groups_out[r];
        s->h_hist_n += n_groups_out[r] * ((int64_t)K[r] + 1);
    }
    if (s->h_goff.ensure(n_rec * 8) || s->h_hoff.ensure(n_rec * 8) || s->h_codes.ensure(s->h_groups * 4) ||
        s->h_hist.ensure(s->h_hist_n * 4))
        return 1;
    HIPCHK(hipMemcpyAsync(s->h_goff.p, goff.data(), n_rec * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->h_hoff.p, hoff.data(), n_rec * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(s->h_hist.p, 0, std::max<int64_t>(s->h_hist_n, 1) * 4, c->stream));
    hipLaunchKernelGGL(k_rep_hist, dim3(n_rec), dim3(REP_THREADS), 0, c->stream, s->r_off.as<int64_t>(),
                       s->r_K.as<int32_t>(), s->r_lab.as<int64_t>(), s->r_cb.as<int64_t>(), id_min, map, n_words,
                       s->h_bits.as<uint32_t>(), s->h_wpre.as<int32_t>(), s->h_goff.as<int64_t>(),
                       s->h_hoff.as<int64_t>(), s->h_codes.as<int32_t>(), s->h_hist.as<int32_t>());
    HIPCHK(hipGetLastError());
    return 0;
}

int scape_hip_report_hist_fetch(scape_hip_ctx *c, int64_t n_groups, int32_t *codes_out, int64_t n_hist,
                                int32_t *hist_out) {
    CTX_ENTER(c);
    ReportState *s = c->rep;
    if (!s || !codes_out || !hist_out) return fail("bad argument");
    if (n_groups != s->h_groups || n_hist != s->h_hist_n)
        return fail("sizes differ from the last scape_hip_report_hist call");
    if (n_groups) HIPCHK(hipMemcpyAsync(codes_out, s->h_codes.p, n_groups * 4, hipMemcpyDeviceToHost, c->stream));
    if (n_hist) HIPCHK(hipMemcpyAsync(hist_out, s->h_hist.p, n_hist * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int scape_hip_report_free(scape_hip_ctx *c) {
    CTX_ENTER(c);
    report_release(c);
    return 0;
}

}  // extern "C"

// ---- permutation test (diff_pa) -------------------------------------------------------------------------------------
// The tested columns are the first n = n1 + n2 columns of the count matrix (population 1, then population 2: the caller's
// id2col puts them there), position j = column j.  Permutation p >= 1 gives population 1 the n1 positions with the
// smallest key(p, j); all arithmetic mod 2^64 (scape_hip.h states the scheme):
//   mix = the splitmix64 finaliser,  h(p, j) = mix(mix(seed + G p) + G (j + 1)),  key = (h & ~0xFFFFFF) | j
#define REP_PERM_G 0x9E3779B97F4A7C15ull
#define REP_PERM_MAX_N (1 << 24)
#define REP_PERM_SLACK 0x1.ffffffffffp-1   // 1 - 2^-40: equal rationals count as ties whatever their rounding

__device__ __forceinline__ unsigned long long rep_mix(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ unsigned long long rep_perm_key(unsigned long long base, int j) {
    return (rep_mix(base + REP_PERM_G * (unsigned long long)(j + 1)) & ~0xFFFFFFull) | (unsigned long long)j;
}

// one workgroup per permutation p_first + blockIdx.x: radix select (most significant byte first, 256-bin LDS histogram,
// keys recomputed in every pass) of the n1-th smallest key, then one pass that writes bit j = (key(j) <= that key) of
// bits[(j / 64) * p_count + blockIdx.x].  Keys are distinct (their low 24 bits are j), so exactly n1 bits are set.
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_mask(int32_t n1, int32_t n, unsigned long long p_first,
                                                               int32_t p_count, unsigned long long seed,
                                                               unsigned long long *__restrict__ bits) {
    __shared__ int hist[256];
    __shared__ unsigned long long sel[2];   // prefix of the key looked for, and its rank among the keys with that prefix
    const unsigned long long base = rep_mix(seed + REP_PERM_G * (p_first + blockIdx.x));
    if (threadIdx.x == 0) {
        sel[0] = 0;
        sel[1] = (unsigned long long)(n1 - 1);
    }
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        hist[threadIdx.x] = 0;
        __syncthreads();
        const unsigned long long prefix = sel[0];
        for (int j = threadIdx.x; j < n; j += REP_THREADS) {
            const unsigned long long k = rep_perm_key(base, j);
            if (pass == 0 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(k >> shift) & 255], 1);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            long long rank = (long long)sel[1];
            int b = 0;
            while (b < 255 && rank >= hist[b]) rank -= hist[b++];
            sel[0] = prefix | ((unsigned long long)b << shift);
            sel[1] = (unsigned long long)rank;
        }
        __syncthreads();
    }
    const unsigned long long thr = sel[0];
    const int lane = threadIdx.x & 63, n_words = (n + 63) >> 6;
    for (int w = threadIdx.x >> 6; w < n_words; w += REP_WAVES) {
        const int j = w * 64 + lane;
        const unsigned long long m = __ballot(j < n && rep_perm_key(base, j) <= thr);
        if (lane == 0) bits[(int64_t)w * p_count + blockIdx.x] = m;
    }
}

// ---- labellings permuted within strata ------------------------------------------------------------------------------
// Stratum s owns the positions [a1, a1 + m1) of population 1 and [a2, a2 + m2) of population 2 (desc[s] = a1, m1, a2,
// m2; a2 already counts from n1).  Permutation p >= 1 gives population 1 the m1 cells of the stratum with the smallest
// key(p, j), j the global position, so with one stratum the bits are k_rep_perm_mask's.  The kernel stores, per
// stratum, the EXCLUSIVE bound of the members' keys: 0 when m1 = 0, 2^64 - 1 when m2 = 0 (j <= 2^24 - 2, so every key
// lies below it), otherwise the m1-th smallest key + 1; the last pass is then k_rep_perm_mask's, with
// key < bound[stratum of j].
#define REP_STRATA_WAVE_MAX 256   // a wave ranks a stratum of up to this many cells in registers (4 keys per lane)

__device__ __forceinline__ int rep_strata_pos(int i, int4 d) { return i < d.y ? d.x + i : d.z + (i - d.y); }

__device__ __forceinline__ unsigned long long rep_readlane64(unsigned long long v, int src) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

// one wave, one stratum of m = d.y + d.w <= 64 KEYS cells, 0 < d.y < m: lane l holds the keys of cells l, 64 + l, ...;
// every key is broadcast in turn and each lane counts the keys below its own.  The cell with d.y - 1 keys below it has
// the d.y-th smallest key.  No LDS, no barrier.
template <int KEYS>
__device__ __forceinline__ void rep_strata_wave(unsigned long long base, int4 d, int lane,
                                                unsigned long long *__restrict__ bound_s) {
    const int m = d.y + d.w;
    unsigned long long k[KEYS];
    int below[KEYS];
#pragma unroll
    for (int c = 0; c < KEYS; ++c) {
        const int i = c * 64 + lane;
        k[c] = i < m ? rep_perm_key(base, rep_strata_pos(i, d)) : ~0ull;   // above every key of a cell
        below[c] = 0;
    }
#pragma unroll
    for (int c2 = 0; c2 < KEYS; ++c2) {
        const int cnt = min(64, m - c2 * 64);
        for (int src = 0; src < cnt; ++src) {
            const unsigned long long other = rep_readlane64(k[c2], src);
#pragma unroll
            for (int c = 0; c < KEYS; ++c) below[c] += other < k[c];
        }
    }
#pragma unroll
    for (int c = 0; c < KEYS; ++c)
        if (c * 64 + lane < m && below[c] == d.y - 1) *bound_s = k[c] + 1;
}

// one workgroup per permutation p_first + blockIdx.x.  order[0 .. n_wave) are the strata a wave settles alone (those
// without a cell of one population, whatever their size, and those of up to REP_STRATA_WAVE_MAX cells), taken by the
// four waves in turn; order[n_wave .. n_strata) are the larger ones, which the whole workgroup takes one after the other
// with k_rep_perm_mask's radix select over the stratum's two ranges.  The select stops at the first byte after which one
// candidate is left (a stratum of m cells needs about log256(m) + 1 of the 8 passes), and one more pass over the
// stratum finds the key that carries the selected prefix.  bound = bound of this launch [permutation][stratum].
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_mask_strata(
    int32_t n, int32_t n_strata, int32_t n_wave, const int4 *__restrict__ desc, const int32_t *__restrict__ order,
    const int32_t *__restrict__ strat_of, unsigned long long p_first, int32_t p_count, unsigned long long seed,
    unsigned long long *__restrict__ bound, unsigned long long *__restrict__ bits) {
    __shared__ __align__(16) int hist[256];
    __shared__ unsigned long long sel[2];   // prefix of the key looked for, and its rank among the keys with that prefix
    __shared__ int sel_cnt;                 // keys that share the prefix
    const unsigned long long base = rep_mix(seed + REP_PERM_G * (p_first + blockIdx.x));
    unsigned long long *__restrict__ bound_p = bound + (int64_t)blockIdx.x * n_strata;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int i = wave; i < n_wave; i += REP_WAVES) {
        const int s = order[i];
        const int4 d = desc[s];
        if (d.y == 0 || d.w == 0) {
            if (lane == 0) bound_p[s] = d.y == 0 ? 0ull : ~0ull;
        } else if (d.y + d.w <= 64) {
            rep_strata_wave<1>(base, d, lane, bound_p + s);
        } else {
            rep_strata_wave<REP_STRATA_WAVE_MAX / 64>(base, d, lane, bound_p + s);
        }
    }
    for (int i = n_wave; i < n_strata; ++i) {
        const int s = order[i];
        const int4 d = desc[s];
        const int m = d.y + d.w;
        unsigned long long prefix = 0;
        int rank = d.y - 1, cnt = m, pass = 0;
        for (; pass < 8 && cnt > 1; ++pass) {
            const int shift = 56 - 8 * pass;
            hist[threadIdx.x] = 0;
            __syncthreads();
            for (int c = threadIdx.x; c < m; c += REP_THREADS) {
                const unsigned long long k = rep_perm_key(base, rep_strata_pos(c, d));
                if (pass == 0 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(k >> shift) & 255], 1);
            }
            __syncthreads();
            if (threadIdx.x < 64) {          // wave 0: the bin that holds the candidate of that rank
                const int4 h = reinterpret_cast<const int4 *>(hist)[lane];
                const int sum = h.x + h.y + h.z + h.w;
                int incl = sum;
                for (int o = 1; o < 64; o <<= 1) {
                    const int y = __shfl_up(incl, o, 64);
                    if (lane >= o) incl += y;
                }
                if (incl - sum <= rank && rank < incl) {     // one lane: the bins are disjoint and hold cnt > rank keys
                    int r = rank - (incl - sum), b = 4 * lane, in_bin = h.x;
                    if (r >= h.x) {
                        r -= h.x, ++b, in_bin = h.y;
                        if (r >= h.y) {
                            r -= h.y, ++b, in_bin = h.z;
                            if (r >= h.z) r -= h.z, ++b, in_bin = h.w;
                        }
                    }
                    sel[0] = prefix | ((unsigned long long)b << shift);
                    sel[1] = (unsigned long long)r;
                    sel_cnt = in_bin;
                }
            }
            __syncthreads();
            prefix = sel[0];
            rank = (int)sel[1];
            cnt = sel_cnt;
        }
        const int known = 64 - 8 * pass;     // pass >= 1: the key's bits above `known` are fixed, and one key has them
        for (int c = threadIdx.x; c < m; c += REP_THREADS) {
            const unsigned long long k = rep_perm_key(base, rep_strata_pos(c, d));
            if ((k >> known) == (prefix >> known)) bound_p[s] = k + 1;
        }
    }
    __syncthreads();                         // this permutation's bounds are stored
    const int n_words = (n + 63) >> 6;
    for (int w = wave; w < n_words; w += REP_WAVES) {
        const int j = w * 64 + lane;
        const unsigned long long m = __ballot(j < n && rep_perm_key(base, j) < bound_p[strat_of[j]]);
        if (lane == 0) bits[(int64_t)w * p_count + blockIdx.x] = m;
    }
}

// one workgroup per kept row i (count row rows[i]): nonzeros among the tested positions, their sum t and the sum over
// positions < n1 (population 1 as observed)
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_rowstat(const int64_t *__restrict__ rows, int32_t n_cols,
                                                                  const int32_t *__restrict__ cnt, int32_t n1, int32_t n,
                                                                  int64_t *__restrict__ nnz, int64_t *__restrict__ t,
                                                                  int64_t *__restrict__ a0) {
    __shared__ long long lds[REP_WAVES];
    const int i = blockIdx.x;
    const int32_t *row = cnt + rows[i] * n_cols;
    long long z = 0, s = 0, a = 0;
    for (int c = threadIdx.x; c < n; c += REP_THREADS) {
        const int v = row[c];
        z += v != 0;
        s += v;
        a += c < n1 ? v : 0;
    }
    z = rep_block_sum<long long, REP_WAVES>(z, lds);
    s = rep_block_sum<long long, REP_WAVES>(s, lds);
    a = rep_block_sum<long long, REP_WAVES>(a, lds);
    if (threadIdx.x == 0) {
        nnz[i] = z;
        t[i] = s;
        a0[i] = a;
    }
}

// one workgroup per kept row: its (position, count) nonzeros, positions ascending, at nz[noff[i] ..]
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_fill(const int64_t *__restrict__ rows, int32_t n_cols,
                                                               const int32_t *__restrict__ cnt, int32_t n,
                                                               const int64_t *__restrict__ noff, uint2 *__restrict__ nz) {
    __shared__ int lds[REP_WAVES];
    const int i = blockIdx.x;
    const int32_t *row = cnt + rows[i] * n_cols;
    uint2 *dst = nz + noff[i];
    int64_t pos = 0;
    for (int base = 0; base < n; base += REP_THREADS) {
        const int c = base + threadIdx.x;
        const int v = c < n ? row[c] : 0;
        int tile;
        const int ex = rep_block_excl<int, REP_WAVES>(v != 0, lds, &tile);
        if (v) dst[pos + ex] = make_uint2((uint32_t)c, (uint32_t)v);
        pos += tile;
    }
}

// the term of S and the usage difference d of one row, from integers: N = a T - t A exactly in 64 bits (both products are
// below 2^62), converted once.  The observed labelling and every permutation go through this one function, with
// contraction off, so equal integers give equal doubles
__device__ __forceinline__ double rep_perm_row(long long a, long long t, long long A, long long T, double *d) {
#pragma clang fp contract(off)
    const long long B = T - A;
    if (A == 0 || B == 0 || t == 0) {
        *d = 0.0;
        return 0.0;
    }
    const double N = (double)(a * T - t * A), Ad = (double)A, Bd = (double)B;
    *d = N / (Ad * Bd);
    return (N * N) / ((double)t * Ad * Bd);
}

// a row's sum over this lane's population 1: the nonzeros are wave-uniform, the lane tests its own permutation's bit.
// Positions ascend within a row, so a mask word is loaded once for all the nonzeros that fall into it
__device__ __forceinline__ int rep_perm_rowsum(const uint2 *__restrict__ nz, int64_t k0, int64_t k1,
                                               const unsigned long long *__restrict__ mb, int64_t pstride) {
    int a = 0, cur = -1;
    unsigned long long w = 0;
    for (int64_t k = k0; k < k1; ++k) {
        const uint2 e = nz[k];
        const int pos = __builtin_amdgcn_readfirstlane((int)e.x), c = __builtin_amdgcn_readfirstlane((int)e.y);
        if ((pos >> 6) != cur) {
            cur = pos >> 6;
            w = mb[(int64_t)cur * pstride];
        }
        a += ((w >> (pos & 63)) & 1) ? c : 0;
    }
    return a;
}

// workgroup = (record recs[blockIdx.x / n_tiles], tile of 256 permutations), one lane per permutation.  a_i(p) of the
// record's rows are kept in LDS as acc[row][lane] (each lane reads and writes its own column: conflict-free, no barrier)
// until A(p) = sum a_i(p) is known; a record with more than `cap` rows is taken in groups of cap rows behind one extra
// walk that forms A(p).  Exceedances are counted per wave (ballot) and added with one atomic per wave and counter.
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_test(
    const unsigned long long *__restrict__ bits, int32_t p_count, int32_t n_tiles, const int32_t *__restrict__ recs,
    const int64_t *__restrict__ roff, const int64_t *__restrict__ noff, const uint2 *__restrict__ nz,
    const int64_t *__restrict__ t, const int64_t *__restrict__ a0, int32_t cap, int32_t *__restrict__ site_ge,
    int32_t *__restrict__ gene_ge, double *__restrict__ stat0) {
#pragma clang fp contract(off)
    extern __shared__ int32_t rep_acc[];
    const int r = recs[blockIdx.x / n_tiles], tile = blockIdx.x % n_tiles;
    const int p = tile * REP_THREADS + threadIdx.x;
    const bool valid = p < p_count;
    const unsigned long long *mb = bits + (valid ? p : p_count - 1);
    int32_t *acc = rep_acc + threadIdx.x;
    const int64_t row0 = roff[r], row1 = roff[r + 1];
    long long T = 0, A0 = 0, A = 0;
    for (int64_t i = row0; i < row1; ++i) {
        T += t[i];
        A0 += a0[i];
    }
    const bool one = row1 - row0 <= cap;
    if (!one)
        for (int64_t i = row0; i < row1; ++i) A += rep_perm_rowsum(nz, noff[i], noff[i + 1], mb, p_count);
    double S = 0.0, S0 = 0.0;
    for (int64_t g0 = row0; g0 < row1; g0 += cap) {
        const int64_t g1 = g0 + cap < row1 ? g0 + cap : row1;
        long long Ag = 0;
        for (int64_t i = g0; i < g1; ++i) {
            const int a = rep_perm_rowsum(nz, noff[i], noff[i + 1], mb, p_count);
            acc[(i - g0) * REP_THREADS] = a;
            Ag += a;
        }
        if (one) A = Ag;
        for (int64_t i = g0; i < g1; ++i) {
            double d, d0;
            S = S + rep_perm_row(acc[(i - g0) * REP_THREADS], t[i], A, T, &d);
            S0 = S0 + rep_perm_row(a0[i], t[i], A0, T, &d0);
            const unsigned long long b = __ballot(valid && fabs(d) >= fabs(d0) * REP_PERM_SLACK);
            if ((threadIdx.x & 63) == 0 && b) atomicAdd(&site_ge[i], __popcll(b));
        }
    }
    const unsigned long long b = __ballot(valid && S >= S0 * REP_PERM_SLACK);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&gene_ge[r], __popcll(b));
    if (tile == 0 && threadIdx.x == 0) stat0[r] = S0;
}

// ---- diff_pa_len: mean pA position ------------------------------------------------------------------------------------
// Row i of a record carries the weight w_i = x_i - min x of its pA position (f64, 0 <= w_i <= span = max x - min x).
// Under a labelling with row sums a_i (population 1) and b_i = t_i - a_i (population 2), A = sum a_i, B = sum b_i:
//   W1 = sum_i (double)a_i * w_i,  W2 = sum_i (double)b_i * w_i   (rows in order; b_i is formed as an integer, NOT
//   W - W1, which cancels when B is small against T),   delta = W1 / A - W2 / B,   0 when A = 0 or B = 0.
// Rounding of the code below (contraction off, unit roundoff u = 2^-53, R rows):
//   * (double)a_i is exact (a_i < 2^31) and a_i * w_i rounds by at most u a_i w_i: all products together by at most
//     u sum a_i w_i <= u A span;
//   * the first addition (0 + product) is exact, each of the other R - 1 rounds by at most u times a partial sum that
//     is at most A span (1 + R u);
//   so |W1 - exact| <= R u A span up to second order.  (double)A is exact and the division rounds by u times a quotient
//   of at most span: each mean is within (R + 1) u span of the mean of the w_i as passed.  The subtraction rounds by at
//   most u span more: |delta - exact| <= (2 R + 3) u span =: e, for the observed labelling and for every permutation.
// The test counts a permutation when |delta(p)| >= |delta(0)| - tol, tol = 2^-40 span, and the threshold's own
// subtraction rounds by at most u span.  A labelling whose exact |delta| reaches the observed one is counted whatever
// the rounding, and one more than 2 tol below it never is, as long as 2 e + u span <= tol.  With R <= 1,024
// (REP_LEN_MAX_ROWS, checked by the entry point) 2 e + u span = (4 R + 7) u span = 4,103 * 2^-53 span, 1.002 * 2^-41
// span: half of tol.  (The host's own rounding of w_i = x_i - min x, at most u span per row and therefore per mean,
// and of tol fit into the other half many times over.)
#define REP_LEN_MAX_ROWS 1024

// one row's share of the four sums of a labelling; the observed labelling and every permutation go through this function
// and rep_len_delta, with contraction off, so equal integers give equal doubles
__device__ __forceinline__ void rep_len_row(int a, int t, double w, double *W1, double *W2, long long *A,
                                            long long *B) {
#pragma clang fp contract(off)
    const int b = t - a;          // a <= t < 2^31 (the entry point refuses a record with 2^31 reads or more)
    *W1 = *W1 + (double)a * w;
    *W2 = *W2 + (double)b * w;
    *A += a;
    *B += b;
}

__device__ __forceinline__ double rep_len_delta(double W1, double W2, long long A, long long B) {
#pragma clang fp contract(off)
    if (A == 0 || B == 0) return 0.0;
    return W1 / (double)A - W2 / (double)B;
}

// workgroup = (record blockIdx.x / n_tiles, tile of 256 permutations), one lane per permutation.  W1, W2, A and B
// accumulate in the one walk over the record's rows (registers only: no LDS, any number of rows in one launch);
// t, a0 and w of a row are wave-uniform loads.  Exceedances are counted per wave (ballot) and added with one atomic
// per wave.
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_len(
    const unsigned long long *__restrict__ bits, int32_t p_count, int32_t n_tiles, const int64_t *__restrict__ roff,
    const int64_t *__restrict__ noff, const uint2 *__restrict__ nz, const int64_t *__restrict__ t,
    const int64_t *__restrict__ a0, const double *__restrict__ w, const double *__restrict__ tol,
    int32_t *__restrict__ n_ge, double *__restrict__ delta0) {
#pragma clang fp contract(off)
    const int r = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles;
    const int p = tile * REP_THREADS + threadIdx.x;
    const bool valid = p < p_count;
    const unsigned long long *mb = bits + (valid ? p : p_count - 1);
    const int64_t row0 = roff[r], row1 = roff[r + 1];
    double W1 = 0.0, W2 = 0.0, V1 = 0.0, V2 = 0.0;
    long long A = 0, B = 0, A0 = 0, B0 = 0;
    for (int64_t i = row0; i < row1; ++i) {
        const int ti = (int)t[i];
        const double wi = w[i];
        rep_len_row(rep_perm_rowsum(nz, noff[i], noff[i + 1], mb, p_count), ti, wi, &W1, &W2, &A, &B);
        rep_len_row((int)a0[i], ti, wi, &V1, &V2, &A0, &B0);
    }
    const double d = rep_len_delta(W1, W2, A, B), d0 = rep_len_delta(V1, V2, A0, B0);
    const unsigned long long b = __ballot(valid && fabs(d) >= fabs(d0) - tol[r]);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&n_ge[r], __popcll(b));
    if (tile == 0 && threadIdx.x == 0) delta0[r] = d0;
}

static const int32_t REP_PERM_CAPS[] = {4, 8, 16, 32, 64};   // rows of a record held in LDS at once (1 KiB each)

// the part scape_hip_report_perm_test and scape_hip_report_perm_len share: the checks (outs_ok = the caller's own
// other pointers are there; max_rec_rows > 0: a record may own at most that many rows; w / tol, when given, must be
// finite and not negative), all of them before anything is queued on the device, then the upload of rows and offsets
// and the compaction of the kept rows to their nonzeros (p_noff / p_nz), with t and a0 of every row on the host
static int rep_perm_prepare(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                            int64_t *t_out, int64_t *a0_out, bool outs_ok, int64_t max_rec_rows, const double *w,
                            const double *tol, int64_t *n_rows_out, int32_t *n_tiles_out) {
    ReportState *s = c->rep;
    if (!s || !s->n_cnt_rows) return fail("scape_hip_report_counts has not been called");
    if (!s->m_count) return fail("scape_hip_report_perm_masks has not been called");
    if (n_rec <= 0 || !rec_row_off || !rows || !t_out || !a0_out || !outs_ok) return fail("bad argument");
    const int32_t n1 = s->m_n1, n = s->m_n1 + s->m_n2;
    if (n > s->n_cols) return fail("the count matrix has fewer columns than the masks have positions");
    if (rec_row_off[0] != 0) return fail("rec_row_off must start at 0");
    for (int r = 0; r < n_rec; ++r)
        if (rec_row_off[r + 1] < rec_row_off[r]) return fail("rec_row_off must be non-decreasing");
    const int64_t n_rows = rec_row_off[n_rec];
    if (n_rows <= 0 || n_rows > INT32_MAX) return fail("rec_row_off must end at the row count, between 1 and 2^31 - 1");
    if (max_rec_rows > 0)
        for (int r = 0; r < n_rec; ++r)
            if (rec_row_off[r + 1] - rec_row_off[r] > max_rec_rows)
                return fail("record " + std::to_string(r) + ": more than " + std::to_string(max_rec_rows) + " rows");
    for (int64_t i = 0; i < n_rows; ++i)
        if (rows[i] < 0 || rows[i] >= s->n_cnt_rows) return fail("row index out of range");
    const int32_t n_tiles = (s->m_count + REP_THREADS - 1) / REP_THREADS;
    if ((int64_t)n_rec * n_tiles > INT32_MAX) return fail("too many records x permutation tiles for one call");
    for (int64_t i = 0; w && i < n_rows; ++i)
        if (!(w[i] >= 0.0) || std::isinf(w[i])) return fail("row weights must be finite and not negative");
    for (int r = 0; tol && r < n_rec; ++r)
        if (!(tol[r] >= 0.0) || std::isinf(tol[r])) return fail("tolerances must be finite and not negative");

    if (s->p_rows.ensure(n_rows * 8) || s->p_roff.ensure(((int64_t)n_rec + 1) * 8) || s->p_nnz.ensure(n_rows * 8) ||
        s->p_noff.ensure((n_rows + 1) * 8) || s->p_t.ensure(n_rows * 8) || s->p_a0.ensure(n_rows * 8) ||
        s->p_gene.ensure((int64_t)n_rec * 4) || s->p_stat0.ensure((int64_t)n_rec * 8))
        return 1;
    HIPCHK(hipMemcpyAsync(s->p_rows.p, rows, n_rows * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->p_roff.p, rec_row_off, ((int64_t)n_rec + 1) * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_rep_perm_rowstat, dim3((uint32_t)n_rows), dim3(REP_THREADS), 0, c->stream,
                       s->p_rows.as<int64_t>(), s->n_cols, s->r_cnt.as<int32_t>(), n1, n, s->p_nnz.as<int64_t>(),
                       s->p_t.as<int64_t>(), s->p_a0.as<int64_t>());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rep_scan, dim3(1), dim3(REP_SCAN_THREADS), 0, c->stream, s->p_nnz.as<int64_t>(),
                       (int32_t)n_rows, s->p_noff.as<int64_t>());
    HIPCHK(hipGetLastError());
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, s->p_noff.as<int64_t>() + n_rows, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(t_out, s->p_t.p, n_rows * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(a0_out, s->p_a0.p, n_rows * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int r = 0; r < n_rec; ++r) {
        int64_t T = 0;
        for (int64_t i = rec_row_off[r]; i < rec_row_off[r + 1]; ++i) T += t_out[i];
        if (T > INT32_MAX) return fail("record " + std::to_string(r) + ": 2^31 or more reads in the tested cells");
    }
    if (s->p_nz.ensure(std::max<int64_t>(total, 1) * 8)) return 1;
    hipLaunchKernelGGL(k_rep_perm_fill, dim3((uint32_t)n_rows), dim3(REP_THREADS), 0, c->stream,
                       s->p_rows.as<int64_t>(), s->n_cols, s->r_cnt.as<int32_t>(), n, s->p_noff.as<int64_t>(),
                       s->p_nz.as<uint2>());
    HIPCHK(hipGetLastError());
    *n_rows_out = n_rows;
    *n_tiles_out = n_tiles;
    return 0;
}

extern "C" {

int scape_hip_report_perm_masks(scape_hip_ctx *c, int32_t n1, int32_t n2, int64_t p_first, int32_t p_count,
                                uint64_t seed) {
    CTX_ENTER(c);
    if (n1 < 1 || n2 < 1) return fail("both populations need at least one cell");
    if ((int64_t)n1 + n2 >= REP_PERM_MAX_N) return fail("n1 + n2 must be below 2^24 (a key keeps the position in 24 bits)");
    if (p_first < 1 || p_count < 1) return fail("p_first and p_count must be at least 1 (permutation 0 is the observed labelling)");
    ReportState *s = report_state(c);
    s->m_count = 0;
    const int32_t n = n1 + n2;
    if (s->m_bits.ensure((int64_t)p_count * ((n + 63) / 64) * 8)) return 1;
    hipLaunchKernelGGL(k_rep_perm_mask, dim3(p_count), dim3(REP_THREADS), 0, c->stream, n1, n,
                       (unsigned long long)p_first, p_count, (unsigned long long)seed,
                       s->m_bits.as<unsigned long long>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    s->m_n1 = n1;
    s->m_n2 = n2;
    s->m_count = p_count;
    return 0;
}

int scape_hip_report_perm_masks_strata(scape_hip_ctx *c, int32_t n_strata, const int32_t *m1, const int32_t *m2,
                                       int64_t p_first, int32_t p_count, uint64_t seed) {
    CTX_ENTER(c);
    if (n_strata < 1 || !m1 || !m2) return fail("at least one stratum, with m1 and m2, is needed");
    int64_t n1 = 0, n2 = 0;
    for (int32_t s = 0; s < n_strata; ++s) {
        if (m1[s] < 0 || m2[s] < 0) return fail("stratum " + std::to_string(s) + ": a negative number of cells");
        if ((int64_t)m1[s] + m2[s] < 1) return fail("stratum " + std::to_string(s) + ": no cell");
        n1 += m1[s];
        n2 += m2[s];
    }
    if (n1 < 1 || n2 < 1) return fail("both populations need at least one cell");
    if (n1 + n2 >= REP_PERM_MAX_N) return fail("n1 + n2 must be below 2^24 (a key keeps the position in 24 bits)");
    if (p_first < 1 || p_count < 1) return fail("p_first and p_count must be at least 1 (permutation 0 is the observed labelling)");
    ReportState *s = report_state(c);
    s->m_count = 0;
    const int32_t n = (int32_t)(n1 + n2);
    // the position ranges of every stratum, the stratum of every position, and the strata in work order
    std::vector<int32_t> desc((size_t)n_strata * 4), order, large, strat_of((size_t)n);
    order.reserve(n_strata);
    int32_t a1 = 0, a2 = (int32_t)n1;
    for (int32_t k = 0; k < n_strata; ++k) {
        int32_t *d = &desc[(size_t)k * 4];
        d[0] = a1, d[1] = m1[k], d[2] = a2, d[3] = m2[k];
        std::fill(strat_of.begin() + a1, strat_of.begin() + a1 + m1[k], k);
        std::fill(strat_of.begin() + a2, strat_of.begin() + a2 + m2[k], k);
        a1 += m1[k];
        a2 += m2[k];
        const bool alone = m1[k] == 0 || m2[k] == 0 || (int64_t)m1[k] + m2[k] <= REP_STRATA_WAVE_MAX;
        (alone ? order : large).push_back(k);
    }
    const int32_t n_wave = (int32_t)order.size();
    order.insert(order.end(), large.begin(), large.end());
    if (s->m_bits.ensure((int64_t)p_count * ((n + 63) / 64) * 8) || s->m_desc.ensure((int64_t)n_strata * 16) ||
        s->m_order.ensure((int64_t)n_strata * 4) || s->m_strat.ensure((int64_t)n * 4) ||
        s->m_bound.ensure((int64_t)p_count * n_strata * 8))
        return 1;
    HIPCHK(hipMemcpyAsync(s->m_desc.p, desc.data(), (int64_t)n_strata * 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->m_order.p, order.data(), (int64_t)n_strata * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->m_strat.p, strat_of.data(), (int64_t)n * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_rep_perm_mask_strata, dim3(p_count), dim3(REP_THREADS), 0, c->stream, n, n_strata, n_wave,
                       s->m_desc.as<int4>(), s->m_order.as<int32_t>(), s->m_strat.as<int32_t>(),
                       (unsigned long long)p_first, p_count, (unsigned long long)seed,
                       s->m_bound.as<unsigned long long>(), s->m_bits.as<unsigned long long>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    s->m_n1 = (int32_t)n1;
    s->m_n2 = (int32_t)n2;
    s->m_count = p_count;
    return 0;
}

int scape_hip_report_perm_bits_get(scape_hip_ctx *c, int32_t p, uint64_t *words_out) {
    CTX_ENTER(c);
    ReportState *s = c->rep;
    if (!s || !s->m_count) return fail("scape_hip_report_perm_masks has not been called");
    if (!words_out) return fail("bad argument");
    if (p < 0 || p >= s->m_count) return fail("p must name a permutation of the last masks call");
    const int32_t n_words = (s->m_n1 + s->m_n2 + 63) / 64;
    HIPCHK(hipMemcpy2DAsync(words_out, 8, s->m_bits.as<unsigned long long>() + p, (size_t)s->m_count * 8, 8, n_words,
                            hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int scape_hip_report_perm_test(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                               int64_t *t_out, int64_t *a0_out, int64_t *site_n_ge_out, double *stat0_out,
                               int64_t *gene_n_ge_out) {
    CTX_ENTER(c);
    int64_t n_rows = 0;
    int32_t n_tiles = 0;
    if (rep_perm_prepare(c, n_rec, rec_row_off, rows, t_out, a0_out, site_n_ge_out && stat0_out && gene_n_ge_out, 0,
                         nullptr, nullptr, &n_rows, &n_tiles))
        return 1;
    ReportState *s = c->rep;
    if (s->p_recs.ensure((int64_t)n_rec * 4) || s->p_site.ensure(n_rows * 4)) return 1;

    // records by LDS class: the smallest cap that holds all their rows (the largest cap takes the rest, in groups)
    const int n_caps = (int)(sizeof(REP_PERM_CAPS) / sizeof(REP_PERM_CAPS[0]));
    std::vector<std::vector<int32_t>> by_cap(n_caps);
    for (int r = 0; r < n_rec; ++r) {
        const int64_t k = rec_row_off[r + 1] - rec_row_off[r];
        int q = 0;
        while (q < n_caps - 1 && k > REP_PERM_CAPS[q]) ++q;
        by_cap[q].push_back(r);
    }
    std::vector<int32_t> recs;
    for (auto &v : by_cap) recs.insert(recs.end(), v.begin(), v.end());
    HIPCHK(hipMemcpyAsync(s->p_recs.p, recs.data(), (int64_t)n_rec * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(s->p_site.p, 0, n_rows * 4, c->stream));
    HIPCHK(hipMemsetAsync(s->p_gene.p, 0, (int64_t)n_rec * 4, c->stream));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_rep_perm_test),
                               hipFuncAttributeMaxDynamicSharedMemorySize, REP_PERM_CAPS[n_caps - 1] * REP_THREADS * 4));
    int64_t first = 0;
    for (int q = 0; q < n_caps; ++q) {
        const int64_t m = (int64_t)by_cap[q].size();
        if (!m) continue;
        const int32_t cap = REP_PERM_CAPS[q];
        hipLaunchKernelGGL(k_rep_perm_test, dim3((uint32_t)(m * n_tiles)), dim3(REP_THREADS),
                           (size_t)cap * REP_THREADS * 4, c->stream, s->m_bits.as<unsigned long long>(), s->m_count,
                           n_tiles, s->p_recs.as<int32_t>() + first, s->p_roff.as<int64_t>(), s->p_noff.as<int64_t>(),
                           s->p_nz.as<uint2>(), s->p_t.as<int64_t>(), s->p_a0.as<int64_t>(), cap,
                           s->p_site.as<int32_t>(), s->p_gene.as<int32_t>(), s->p_stat0.as<double>());
        HIPCHK(hipGetLastError());
        first += m;
    }
    std::vector<int32_t> site(n_rows), gene(n_rec);
    HIPCHK(hipMemcpyAsync(site.data(), s->p_site.p, n_rows * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(gene.data(), s->p_gene.p, (int64_t)n_rec * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(stat0_out, s->p_stat0.p, (int64_t)n_rec * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < n_rows; ++i) site_n_ge_out[i] += site[i];
    for (int r = 0; r < n_rec; ++r) gene_n_ge_out[r] += gene[r];
    return 0;
}

int scape_hip_report_perm_len(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                              const double *w, const double *tol, int64_t *t_out, int64_t *a0_out, double *delta0_out,
                              int64_t *n_ge_out) {
    CTX_ENTER(c);
    int64_t n_rows = 0;
    int32_t n_tiles = 0;
    if (rep_perm_prepare(c, n_rec, rec_row_off, rows, t_out, a0_out, w && tol && delta0_out && n_ge_out,
                         REP_LEN_MAX_ROWS, w, tol, &n_rows, &n_tiles))
        return 1;
    ReportState *s = c->rep;
    if (s->l_w.ensure(n_rows * 8) || s->l_tol.ensure((int64_t)n_rec * 8)) return 1;
    HIPCHK(hipMemcpyAsync(s->l_w.p, w, n_rows * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->l_tol.p, tol, (int64_t)n_rec * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(s->p_gene.p, 0, (int64_t)n_rec * 4, c->stream));
    hipLaunchKernelGGL(k_rep_perm_len, dim3((uint32_t)((int64_t)n_rec * n_tiles)), dim3(REP_THREADS), 0, c->stream,
                       s->m_bits.as<unsigned long long>(), s->m_count, n_tiles, s->p_roff.as<int64_t>(),
                       s->p_noff.as<int64_t>(), s->p_nz.as<uint2>(), s->p_t.as<int64_t>(), s->p_a0.as<int64_t>(),
                       s->l_w.as<double>(), s->l_tol.as<double>(), s->p_gene.as<int32_t>(), s->p_stat0.as<double>());
    HIPCHK(hipGetLastError());
    std::vector<int32_t> ge(n_rec);
    HIPCHK(hipMemcpyAsync(ge.data(), s->p_gene.p, (int64_t)n_rec * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(delta0_out, s->p_stat0.p, (int64_t)n_rec * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int r = 0; r < n_rec; ++r) n_ge_out[r] += ge[r];
    return 0;
}

}  // extern "C"

// ---- G-way labellings (diff_pa_groups) --------------------------------------------------------------------------------
// G = 2..64 populations of sizes n_0 .. n_{G-1}, n = sum n_g tested columns in front of the count matrix, population 0's
// first.  Permutation p >= 1 ranks the n keys key(p, j) (the key of diff_pa, unchanged) and gives the n_0 smallest to
// group 0, the next n_1 to group 1, ...: with c_h = n_0 + .. + n_{h-1} and cut_h = the key of rank c_h - 1 (the largest
// key of the groups below h), h = 1..G-1, the group of position j is #{h : cut_h < key(p, j)}.  With G = 2, group 0 is
// population 1 of k_rep_perm_mask.
//
// The statistic, per record with R kept rows: a_ig = the sum of row i over group g, A_g = sum_i a_ig, t_i = sum_g a_ig,
// T = sum_i t_i < 2^31, N_ig = a_ig T - t_i A_g exactly in 64 bits (both products are below 2^62),
//   s_i = sum_{g : A_g > 0} N_ig^2 / A_g   (groups in order)        the site's statistic
//   S   = sum_i s_i / (T t_i)              (rows in order)          Pearson's chi-square of the rows x G table
// Every term is positive or zero; no difference is formed in f64.
// Rounding of the code below (contraction off, unit roundoff u = 2^-53, first order in u):
//   * (double)N_ig rounds by u (|N| < 2^62), its square by 2 u + u, the division by the exact (double)A_g by u more:
//     a term is within 4 u of N^2 / A, relatively;
//   * the first addition of a row (0 + term) is exact, each of the other G - 1 rounds by at most u times a partial sum
//     of positive terms: s_i is within (G + 3) u;
//   * (double)T and (double)t_i are exact, their product rounds by u, the division by u: a row's share s_i / (T t_i) is
//     within (G + 5) u; the first of the R additions is exact, the others round by u each: S is within
//     e = (R + G + 4) u.
// The sums are NESTED (groups inside a row, rows inside the record), so the error grows with R + G.  It would grow
// with R x G only if all R x G terms went through one running sum, which neither the definition above nor this code
// does; a bound on the product (R x G <= 4,000 or so) is sufficient but far from necessary.
// The test counts a permutation when S(p) >= S(0) (1 - 2^-40); 1 - 2^-40 is a double and the product rounds by u.
// Two labellings with equal rationals are both within e of it, so the permuted one is counted when
// 1 - e >= (1 + e)(1 - 2^-40)(1 + u), and a labelling at S(0) (1 - 2^-39) or below is never counted when
// (1 - 2^-39)(1 + e) < (1 - e)(1 - 2^-40)(1 - u): both hold when 2 e + u < 2^-40 = 8,192 u, up to terms of second
// order (e^2 < 2^-80).  With R + G <= 4,000 (REP_GROUPS_MAX_ROWS_AND_GROUPS, checked by the entry point)
// 2 e + u <= 8,009 u: 183 u to spare.  The site statistic s_i has the error (G + 3) u <= 67 u and needs no bound.
#define REP_GROUPS_MAX 64
#define REP_GROUPS_MAX_ROWS_AND_GROUPS 4000

// the key of rank `rank` among key(base, j), j = 0 .. n-1, n >= 2, for the whole workgroup (every thread calls, every
// thread gets the key): k_rep_perm_mask's radix select in the form k_rep_perm_mask_strata gives it - wave 0 finds the
// bin, and the select stops at the first byte after which one candidate is left (about log256(n) + 1 of the 8
// passes); one more pass finds the key that carries the selected prefix
__device__ __forceinline__ unsigned long long rep_select_key(unsigned long long base, int n, int rank, int *hist,
                                                             unsigned long long *sel, int *sel_cnt) {
    const int lane = threadIdx.x & 63;
    unsigned long long prefix = 0;
    int cnt = n, pass = 0;
    for (; pass < 8 && cnt > 1; ++pass) {
        const int shift = 56 - 8 * pass;
        hist[threadIdx.x] = 0;
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += REP_THREADS) {
            const unsigned long long k = rep_perm_key(base, j);
            if (pass == 0 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(k >> shift) & 255], 1);
        }
        __syncthreads();
        if (threadIdx.x < 64) {              // wave 0: the bin that holds the candidate of that rank
            const int4 h = reinterpret_cast<const int4 *>(hist)[lane];
            const int sum = h.x + h.y + h.z + h.w;
            int incl = sum;
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(incl, o, 64);
                if (lane >= o) incl += y;
            }
            if (incl - sum <= rank && rank < incl) {     // one lane: the bins are disjoint and hold cnt > rank keys
                int r = rank - (incl - sum), b = 4 * lane, in_bin = h.x;
                if (r >= h.x) {
                    r -= h.x, ++b, in_bin = h.y;
                    if (r >= h.y) {
                        r -= h.y, ++b, in_bin = h.z;
                        if (r >= h.z) r -= h.z, ++b, in_bin = h.w;
                    }
                }
                sel[0] = prefix | ((unsigned long long)b << shift);
                sel[1] = (unsigned long long)r;
                *sel_cnt = in_bin;
            }
        }
        __syncthreads();
        prefix = sel[0];
        rank = (int)sel[1];
        cnt = *sel_cnt;
    }
    const int known = 64 - 8 * pass;         // n >= 2, so pass >= 1: the bits above `known` are fixed, one key has them
    __syncthreads();                         // every thread holds the prefix: sel[0] may now take the key
    for (int j = threadIdx.x; j < n; j += REP_THREADS) {
        const unsigned long long k = rep_perm_key(base, j);
        if ((k >> known) == (prefix >> known)) sel[0] = k;
    }
    __syncthreads();
    const unsigned long long key = sel[0];
    __syncthreads();                         // the next select writes sel again
    return key;
}

// one workgroup per permutation p_first + blockIdx.x: the G - 1 cut keys (rank_of_cut[h] = c_{h+1} - 1, ascending, so
// the cut keys ascend too), then one pass that counts, per position, the cut keys below its key (binary search in LDS)
// and writes that group as the byte labels[j * p_count + blockIdx.x].  A workgroup's bytes lie p_count apart: the
// workgroups of neighbouring permutations fill a cache line between them.
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_labels(int32_t n_groups, const int32_t *__restrict__ rank_of_cut,
                                                                 int32_t n, unsigned long long p_first, int32_t p_count,
                                                                 unsigned long long seed, uint8_t *__restrict__ labels) {
    __shared__ __align__(16) int hist[256];
    __shared__ unsigned long long sel[2];
    __shared__ int sel_cnt;
    __shared__ unsigned long long cuts[REP_GROUPS_MAX - 1];
    const unsigned long long base = rep_mix(seed + REP_PERM_G * (p_first + blockIdx.x));
    const int n_cuts = n_groups - 1;
    for (int h = 0; h < n_cuts; ++h) {
        const unsigned long long k = rep_select_key(base, n, rank_of_cut[h], hist, sel, &sel_cnt);
        if (threadIdx.x == 0) cuts[h] = k;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += REP_THREADS) {
        const unsigned long long k = rep_perm_key(base, j);
        int lo = 0, hi = n_cuts;             // lo = cut keys below k
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cuts[mid] < k) lo = mid + 1;
            else hi = mid;
        }
        labels[(int64_t)j * p_count + blockIdx.x] = (uint8_t)lo;
    }
}

// one workgroup per kept row i (count row rows[i]): a0[i * n_groups + g] = its sum over group g as observed (the columns
// [seg_off[g], seg_off[g + 1]); wave w takes groups w, w + REP_WAVES, ...), t[i] = their sum, nnz[i] = its nonzeros
__global__ __launch_bounds__(REP_THREADS) void k_rep_groups_rowstat(const int64_t *__restrict__ rows, int32_t n_cols,
                                                                    const int32_t *__restrict__ cnt, int32_t n_groups,
                                                                    const int32_t *__restrict__ seg_off,
                                                                    int64_t *__restrict__ nnz, int64_t *__restrict__ t,
                                                                    int64_t *__restrict__ a0) {
    __shared__ long long sum_g[REP_GROUPS_MAX], nz_g[REP_GROUPS_MAX];
    const int i = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int32_t *row = cnt + rows[i] * n_cols;
    for (int g = w; g < n_groups; g += REP_WAVES) {
        long long s = 0, z = 0;
        for (int c = seg_off[g] + lane; c < seg_off[g + 1]; c += 64) {
            const int v = row[c];
            s += v;
            z += v != 0;
        }
        for (int o = 32; o > 0; o >>= 1) {
            s += __shfl_xor(s, o, 64);
            z += __shfl_xor(z, o, 64);
        }
        if (lane == 0) {
            sum_g[g] = s;
            nz_g[g] = z;
            a0[(int64_t)i * n_groups + g] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long s = 0, z = 0;
        for (int g = 0; g < n_groups; ++g) {
            s += sum_g[g];
            z += nz_g[g];
        }
        t[i] = s;
        nnz[i] = z;
    }
}

// s_i of one row under one labelling: a[g * stride] = a_ig, A[g * stride] = A_g.  The observed labelling (64-bit sums
// from global memory) and every permutation (32-bit sums in LDS) go through this function and rep_groups_share, with
// contraction off; every operation is a correctly rounded IEEE one, so equal integers give equal doubles
template <typename I>
__device__ __forceinline__ double rep_groups_site(const I *a, const I *A, int stride, int n_groups, long long t,
                                                  long long T) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int g = 0; g < n_groups; ++g) {
        const long long Ag = A[g * stride];
        if (Ag > 0) {
            const double N = (double)((long long)a[g * stride] * T - t * Ag);
            s = s + (N * N) / (double)Ag;
        }
    }
    return s;
}

__device__ __forceinline__ double rep_groups_share(double s, long long t, long long T) {
#pragma clang fp contract(off)
    return t > 0 ? s / ((double)T * (double)t) : 0.0;
}

// one workgroup per record: the observed labelling.  s0[i] = s_i(0), share0[i] = s_i(0) / (T t_i), stat0[r] = S(0),
// the shares added in row order by one thread, as a lane of k_rep_perm_groups adds them
__global__ __launch_bounds__(REP_THREADS) void k_rep_groups_obs(const int64_t *__restrict__ roff,
                                                                const int64_t *__restrict__ t,
                                                                const int64_t *__restrict__ a0, int32_t n_groups,
                                                                double *__restrict__ s0, double *__restrict__ share0,
                                                                double *__restrict__ stat0) {
#pragma clang fp contract(off)
    __shared__ long long A0[REP_GROUPS_MAX];
    __shared__ long long T0;
    const int r = blockIdx.x;
    const int64_t row0 = roff[r], row1 = roff[r + 1];
    if (threadIdx.x < n_groups) {
        long long A = 0;
        for (int64_t i = row0; i < row1; ++i) A += a0[i * n_groups + threadIdx.x];
        A0[threadIdx.x] = A;
    }
    if (threadIdx.x == REP_THREADS - 1) {
        long long T = 0;
        for (int64_t i = row0; i < row1; ++i) T += t[i];
        T0 = T;
    }
    __syncthreads();
    const long long T = T0;
    for (int64_t i = row0 + threadIdx.x; i < row1; i += REP_THREADS) {
        const double s = rep_groups_site<long long>(reinterpret_cast<const long long *>(a0) + i * n_groups, A0, 1,
                                                    n_groups, t[i], T);
        s0[i] = s;
        share0[i] = rep_groups_share(s, t[i], T);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double S = 0.0;
        for (int64_t i = row0; i < row1; ++i) S = S + share0[i];
        stat0[r] = S;
    }
}

// the nonzeros nz[k0 .. k1) added to acc[group][lane] under this lane's labelling (lb = the lane's byte of position 0,
// the positions pstride bytes apart).  The nonzeros are wave-uniform.  Four at a time: their label bytes are loaded
// before the first addition waits for one.  The addition is an LDS atomic whose result is not used - one ds_add
// without a return value in place of a read, an add and a write that would wait for each other; no other lane touches
// the address
__device__ __forceinline__ void rep_groups_walk(const uint2 *__restrict__ nz, int64_t k0, int64_t k1,
                                                const uint8_t *__restrict__ lb, int64_t pstride, int32_t *acc) {
    int64_t k = k0;
    for (; k + 4 <= k1; k += 4) {
        int c[4], g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint2 e = nz[k + u];
            c[u] = __builtin_amdgcn_readfirstlane((int)e.y);
            g[u] = lb[(int64_t)__builtin_amdgcn_readfirstlane((int)e.x) * pstride];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) atomicAdd(&acc[g[u] * REP_THREADS], c[u]);
    }
    for (; k < k1; ++k) {
        const uint2 e = nz[k];
        const int c = __builtin_amdgcn_readfirstlane((int)e.y);
        atomicAdd(&acc[(int)lb[(int64_t)__builtin_amdgcn_readfirstlane((int)e.x) * pstride] * REP_THREADS], c);
    }
}

// workgroup = (record blockIdx.x / n_tiles, tile of 256 permutations), one lane per permutation; the nonzeros are
// wave-uniform, the lane reads its own permutation's byte of the nonzero's position (neighbouring lanes, neighbouring
// bytes) and adds the count to acc[group][lane] in LDS: dword address group * 256 + lane, so the bank is lane mod 32
// whatever the group and the lanes of a 32-lane access group never meet on one; each lane owns its column and no
// barrier is needed (rep_groups_walk).  LDS holds A_g(p) (first walk over all the record's
// nonzeros) and a_ig(p) of the current row (second walk, row by row): 2 x n_groups x 1 KiB.  Exceedances are counted
// per wave (ballot) and added with one atomic per wave and counter.
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_groups(
    const uint8_t *__restrict__ labels, int32_t p_count, int32_t n_tiles, int32_t n_groups,
    const int64_t *__restrict__ roff, const int64_t *__restrict__ noff, const uint2 *__restrict__ nz,
    const int64_t *__restrict__ t, const double *__restrict__ s0, const double *__restrict__ stat0,
    int32_t *__restrict__ site_ge, int32_t *__restrict__ gene_ge) {
#pragma clang fp contract(off)
    extern __shared__ int32_t rep_acc[];
    const int r = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles;
    const int p = tile * REP_THREADS + threadIdx.x;
    const bool valid = p < p_count;
    const uint8_t *lb = labels + (valid ? p : p_count - 1);
    int32_t *accA = rep_acc + threadIdx.x, *acca = accA + n_groups * REP_THREADS;
    const int64_t row0 = roff[r], row1 = roff[r + 1];
    long long T = 0;
    for (int64_t i = row0; i < row1; ++i) T += t[i];
    for (int g = 0; g < n_groups; ++g) accA[g * REP_THREADS] = 0;
    rep_groups_walk(nz, noff[row0], noff[row1], lb, p_count, accA);
    double S = 0.0;
    for (int64_t i = row0; i < row1; ++i) {
        for (int g = 0; g < n_groups; ++g) acca[g * REP_THREADS] = 0;
        rep_groups_walk(nz, noff[i], noff[i + 1], lb, p_count, acca);
        const long long ti = t[i];
        const double s = rep_groups_site<int32_t>(acca, accA, REP_THREADS, n_groups, ti, T);
        S = S + rep_groups_share(s, ti, T);
        const unsigned long long b = __ballot(valid && s >= s0[i] * REP_PERM_SLACK);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(&site_ge[i], __popcll(b));
    }
    const unsigned long long b = __ballot(valid && S >= stat0[r] * REP_PERM_SLACK);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&gene_ge[r], __popcll(b));
}

extern "C" {

int scape_hip_report_perm_labels(scape_hip_ctx *c, int32_t n_groups, const int32_t *sizes, int64_t p_first,
                                 int32_t p_count, uint64_t seed) {
    CTX_ENTER(c);
    if (n_groups < 2 || n_groups > REP_GROUPS_MAX)
        return fail("n_groups must lie in 2 .. " + std::to_string(REP_GROUPS_MAX));
    if (!sizes) return fail("bad argument");
    int64_t n = 0;
    for (int32_t g = 0; g < n_groups; ++g) {
        if (sizes[g] < 1) return fail("group " + std::to_string(g) + ": every group needs at least one cell");
        n += sizes[g];
    }
    if (n >= REP_PERM_MAX_N) return fail("the groups' cells must number below 2^24 (a key keeps the position in 24 bits)");
    if (p_first < 1 || p_count < 1) return fail("p_first and p_count must be at least 1 (permutation 0 is the observed labelling)");
    ReportState *s = report_state(c);
    s->q_count = 0;
    std::vector<int32_t> rank_of_cut(n_groups - 1);
    int32_t below = 0;
    for (int32_t h = 0; h + 1 < n_groups; ++h) {
        below += sizes[h];
        rank_of_cut[h] = below - 1;
    }
    if (s->q_lab.ensure((int64_t)p_count * n) || s->q_cut.ensure((int64_t)(n_groups - 1) * 4)) return 1;
    HIPCHK(hipMemcpyAsync(s->q_cut.p, rank_of_cut.data(), (int64_t)(n_groups - 1) * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_rep_perm_labels, dim3(p_count), dim3(REP_THREADS), 0, c->stream, n_groups,
                       s->q_cut.as<int32_t>(), (int32_t)n, (unsigned long long)p_first, p_count,
                       (unsigned long long)seed, s->q_lab.as<uint8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    s->q_sizes.assign(sizes, sizes + n_groups);
    s->q_n = (int32_t)n;
    s->q_count = p_count;
    return 0;
}

int scape_hip_report_perm_labels_get(scape_hip_ctx *c, int32_t p, uint8_t *labels_out) {
    CTX_ENTER(c);
    ReportState *s = c->rep;
    if (!s || !s->q_count) return fail("scape_hip_report_perm_labels has not been called");
    if (!labels_out) return fail("bad argument");
    if (p < 0 || p >= s->q_count) return fail("p must name a permutation of the last labels call");
    HIPCHK(hipMemcpy2DAsync(labels_out, 1, s->q_lab.as<uint8_t>() + p, (size_t)s->q_count, 1, (size_t)s->q_n,
                            hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int scape_hip_report_perm_groups(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                 int32_t n_groups, const int32_t *seg_off, int64_t *t_out, int64_t *a0_out,
                                 int64_t *site_n_ge_out, double *stat0_out, double *site_stat0_out,
                                 int64_t *gene_n_ge_out) {
    CTX_ENTER(c);
    ReportState *s = c->rep;
    if (!s || !s->n_cnt_rows) return fail("scape_hip_report_counts has not been called");
    if (!s->q_count) return fail("scape_hip_report_perm_labels has not been called");
    if (n_rec <= 0 || !rec_row_off || !rows || !seg_off || !t_out || !a0_out || !site_n_ge_out || !stat0_out ||
        !site_stat0_out || !gene_n_ge_out)
        return fail("bad argument");
    if (n_groups != (int32_t)s->q_sizes.size()) return fail("n_groups differs from the last scape_hip_report_perm_labels call");
    if (seg_off[0] != 0) return fail("seg_off must start at 0 (position j is column j)");
    for (int32_t g = 0; g < n_groups; ++g)
        if (seg_off[g + 1] - seg_off[g] != s->q_sizes[g])
            return fail("group " + std::to_string(g) + ": seg_off differs from the sizes of the last scape_hip_report_perm_labels call");
    const int32_t n = s->q_n;
    if (n > s->n_cols) return fail("the count matrix has fewer columns than the labels have positions");
    if (rec_row_off[0] != 0) return fail("rec_row_off must start at 0");
    for (int r = 0; r < n_rec; ++r)
        if (rec_row_off[r + 1] < rec_row_off[r]) return fail("rec_row_off must be non-decreasing");
    const int64_t n_rows = rec_row_off[n_rec];
    if (n_rows <= 0 || n_rows > INT32_MAX) return fail("rec_row_off must end at the row count, between 1 and 2^31 - 1");
    for (int r = 0; r < n_rec; ++r)
        if (rec_row_off[r + 1] - rec_row_off[r] + n_groups > REP_GROUPS_MAX_ROWS_AND_GROUPS)
            return fail("record " + std::to_string(r) + ": " + std::to_string(rec_row_off[r + 1] - rec_row_off[r]) +
                        " rows and " + std::to_string(n_groups) + " groups, together more than " +
                        std::to_string(REP_GROUPS_MAX_ROWS_AND_GROUPS) + " (the rounding bound of the statistic)");
    for (int64_t i = 0; i < n_rows; ++i)
        if (rows[i] < 0 || rows[i] >= s->n_cnt_rows) return fail("row index out of range");
    const int32_t n_tiles = (s->q_count + REP_THREADS - 1) / REP_THREADS;
    if ((int64_t)n_rec * n_tiles > INT32_MAX) return fail("too many records x permutation tiles for one call");

    if (s->p_rows.ensure(n_rows * 8) || s->p_roff.ensure(((int64_t)n_rec + 1) * 8) || s->p_nnz.ensure(n_rows * 8) ||
        s->p_noff.ensure((n_rows + 1) * 8) || s->p_t.ensure(n_rows * 8) || s->q_a0.ensure(n_rows * n_groups * 8) ||
        s->q_seg.ensure(((int64_t)n_groups + 1) * 4) || s->q_s0.ensure(n_rows * 8) || s->q_share.ensure(n_rows * 8) ||
        s->p_site.ensure(n_rows * 4) || s->p_gene.ensure((int64_t)n_rec * 4) || s->p_stat0.ensure((int64_t)n_rec * 8))
        return 1;
    HIPCHK(hipMemcpyAsync(s->p_rows.p, rows, n_rows * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->p_roff.p, rec_row_off, ((int64_t)n_rec + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->q_seg.p, seg_off, ((int64_t)n_groups + 1) * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_rep_groups_rowstat, dim3((uint32_t)n_rows), dim3(REP_THREADS), 0, c->stream,
                       s->p_rows.as<int64_t>(), s->n_cols, s->r_cnt.as<int32_t>(), n_groups, s->q_seg.as<int32_t>(),
                       s->p_nnz.as<int64_t>(), s->p_t.as<int64_t>(), s->q_a0.as<int64_t>());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rep_scan, dim3(1), dim3(REP_SCAN_THREADS), 0, c->stream, s->p_nnz.as<int64_t>(),
                       (int32_t)n_rows, s->p_noff.as<int64_t>());
    HIPCHK(hipGetLastError());
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, s->p_noff.as<int64_t>() + n_rows, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(t_out, s->p_t.p, n_rows * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(a0_out, s->q_a0.p, n_rows * n_groups * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int r = 0; r < n_rec; ++r) {
        int64_t T = 0;
        for (int64_t i = rec_row_off[r]; i < rec_row_off[r + 1]; ++i) T += t_out[i];
        if (T > INT32_MAX) return fail("record " + std::to_string(r) + ": 2^31 or more reads in the tested cells");
    }
    if (s->p_nz.ensure(std::max<int64_t>(total, 1) * 8)) return 1;
    hipLaunchKernelGGL(k_rep_perm_fill, dim3((uint32_t)n_rows), dim3(REP_THREADS), 0, c->stream,
                       s->p_rows.as<int64_t>(), s->n_cols, s->r_cnt.as<int32_t>(), n, s->p_noff.as<int64_t>(),
                       s->p_nz.as<uint2>());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rep_groups_obs, dim3((uint32_t)n_rec), dim3(REP_THREADS), 0, c->stream, s->p_roff.as<int64_t>(),
                       s->p_t.as<int64_t>(), s->q_a0.as<int64_t>(), n_groups, s->q_s0.as<double>(),
                       s->q_share.as<double>(), s->p_stat0.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(s->p_site.p, 0, n_rows * 4, c->stream));
    HIPCHK(hipMemsetAsync(s->p_gene.p, 0, (int64_t)n_rec * 4, c->stream));
    const size_t lds = (size_t)2 * n_groups * REP_THREADS * 4;   // above 64 KiB a kernel needs the attribute
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_rep_perm_groups),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 2 * REP_GROUPS_MAX * REP_THREADS * 4));
    hipLaunchKernelGGL(k_rep_perm_groups, dim3((uint32_t)((int64_t)n_rec * n_tiles)), dim3(REP_THREADS), lds, c->stream,
                       s->q_lab.as<uint8_t>(), s->q_count, n_tiles, n_groups, s->p_roff.as<int64_t>(),
                       s->p_noff.as<int64_t>(), s->p_nz.as<uint2>(), s->p_t.as<int64_t>(), s->q_s0.as<double>(),
                       s->p_stat0.as<double>(), s->p_site.as<int32_t>(), s->p_gene.as<int32_t>());
    HIPCHK(hipGetLastError());
    std::vector<int32_t> site(n_rows), gene(n_rec);
    HIPCHK(hipMemcpyAsync(site.data(), s->p_site.p, n_rows * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(gene.data(), s->p_gene.p, (int64_t)n_rec * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(stat0_out, s->p_stat0.p, (int64_t)n_rec * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(site_stat0_out, s->q_share.p, n_rows * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < n_rows; ++i) site_n_ge_out[i] += site[i];
    for (int r = 0; r < n_rec; ++r) gene_n_ge_out[r] += gene[r];
    return 0;
}

}  // extern "C"
