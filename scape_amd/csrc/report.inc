// report.inc - the count matrix of merge_pa's output on the device and the reporting stages that read it (included at
// the end of scape_hip.hip, before perm.inc, which holds the permutation tests on the same counts).
//
//   ex_pa_cnt_mat   reference utils.py:438-553: per record, a pivot of (label < K) x barcode read counts, padded to every
//                   barcode of barcode_index.csv and written as a dense, fully quoted CSV row per label.
//   cal_exp_pa_len  reference utils.py:319-427 / apa_core.py:1038-1063: per record and cell cluster, the label histogram
//                   that exp_pa_len turns into an expected pA length.
//   ex_pa_pseudobulk  the count rows summed over cell groups.
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
// Cluster names, their order and the floating-point finish of exp_pa_len stay on the host (scape_amd/report.py).

#define REP_THREADS 256
#define REP_WAVES (REP_THREADS / 64)
#define REP_SCAN_THREADS 1024
#define REP_ZERO_FIELD 6   // ,"0.0"

// What a builder of perm.inc left: its entry point and its noun for messages, the positions, the permutations of the
// chunk (0 until a call has succeeded) and, for a test on groups, their sizes.  ready() opens a test entry point
struct RepLabellings {
    const char *builder, *what;
    int32_t n = 0, count = 0;
    std::vector<int32_t> sizes;
    int built() const { return count ? 0 : fail(std::string(builder) + " has not been called"); }
    int ready(int64_t cnt_rows) const { return cnt_rows ? built() : fail("scape_hip_report_counts has not been called"); }
    int holds(int32_t p) const {
        return p >= 0 && p < count ? 0 : fail("p must name a permutation of the last " + std::string(what) + " call");
    }
};

struct ReportState {
    // counts of the last scape_hip_report_counts call
    DevBuf r_lab, r_cb, r_off, r_K, r_rowbase, r_map, r_cnt, r_tot, r_cflag, r_err;
    int32_t n_cols = 0;
    int64_t n_cnt_rows = 0;
    // ex_pa_usage_mat (usage_mat.inc): per record of the last scape_hip_report_usage_totals call and column, the reads
    // with label < K ([record][column], int32); the records' first count rows and K on the device and on the host; the
    // number of those records, 0 until that call has followed the last counts call
    DevBuf u_tot, u_row0, u_K;
    std::vector<int64_t> u_rows;
    std::vector<int32_t> u_Ks;
    int32_t u_n_rec = 0;
    // histograms of the last scape_hip_report_hist call
    DevBuf h_bits, h_wpre, h_nloc, h_goff, h_hoff, h_codes, h_hist;
    std::vector<int64_t> goff, hoff;   // host side of h_goff / h_hoff: alive until the queued copies have run
    int64_t h_groups = 0, h_hist_n = 0;
    // segment sums of the last scape_hip_report_group_sums call
    DevBuf g_rows, g_off, g_sum, g_nz;
    // the permutation tests (perm.inc), per builder what it left.  First the buffers of rep_perm_prepare / rep_perm_count
    DevBuf p_rows, p_roff, p_nnz, p_noff, p_nz, p_t, p_a0, p_recs, p_site, p_gene, p_stat0;
    // diff_pa, diff_pa_len: membership bits of the last scape_hip_report_perm_masks[_strata] call ([column word]
    // [permutation]); what they are built from: (a1, m1, a2, m2) per stratum, the strata in work order, the stratum of
    // every position and the exclusive key bound per (permutation, stratum)
    RepLabellings masks{"scape_hip_report_perm_masks", "masks"};
    DevBuf m_bits, m_desc, m_order, m_strat, m_bound;
    DevBuf l_w, l_tol;                 // diff_pa_len: row weights and record tolerances of scape_hip_report_perm_len
    // diff_pa_groups: the group of every (position, permutation) of the last scape_hip_report_perm_labels call
    // ([position][permutation], one byte each), the ranks of its cut keys, and the buffers of
    // scape_hip_report_perm_groups that scape_hip_report_perm_test has no counterpart of
    RepLabellings labels{"scape_hip_report_perm_labels", "labels"};
    DevBuf q_lab, q_cut, q_seg, q_a0, q_s0, q_share;
    // diff_pa_len_groups: the integer row positions and (tolD, told) per record of scape_hip_report_perm_len_groups,
    // and per record (Q, T), (double)Q / (double)T and the G observed d_g
    DevBuf v_q, v_tol, v_qt, v_mean, v_d0;
    // diff_pa_pairs: the membership bits of every (pair, permutation) of the last scape_hip_report_perm_pair_masks call
    // ([pair's word offset + word][permutation]), the exclusive key bound per (pair, permutation), (g, h, n_g, word
    // offset) per pair on the device and on the host, and per kept row and group the first nonzero at or beyond the
    // group's segment (scape_hip_report_perm_pairs)
    RepLabellings pair_masks{"scape_hip_report_perm_pair_masks", "pair masks"};
    DevBuf x_bits, x_bound, x_desc, x_seg;
    std::vector<int32_t> x_pairs;
    // diff_pa_markers: the membership bits of every (marker, permutation) of the last scape_hip_report_perm_marker_masks
    // call ([marker * words + word][permutation], the bits in column order), the exclusive key bound per (marker,
    // permutation), the segment offsets and the rank of every position's column on the device; sizes = those of the
    // markers with the number of other cells behind them
    RepLabellings marker_masks{"scape_hip_report_perm_marker_masks", "marker masks"};
    DevBuf k_bits, k_bound, k_seg, k_rank;
    // diff_pa_trend: the score of every (position, permutation) of the last scape_hip_report_perm_scores call
    // ([position][permutation], a halfword each), per permutation of that call the positions sorted into key buckets, the
    // observed scores, their largest, and per kept row of scape_hip_report_perm_trend s_i(0) and sum_j c_ij q_j^2;
    // diff_pa_len_trend: per record of scape_hip_report_perm_len_trend T, Sx, Sz(0), Sxz(0) and the two halves of C(0)
    RepLabellings scores{"scape_hip_report_perm_scores", "scores"};
    DevBuf t_scores, t_members, t_q, t_s0, t_sq0, t_lrec;
    int32_t m_n1 = 0, t_qspan = 0;     // population 1's cells of the masks; the largest observed score
    // boot_pa_len: the multiplicity of every (position, replicate) of the last scape_hip_report_boot_mult call
    // ([position][replicate], one byte each) and the first replicate of that call; the cell of every position; the
    // integer row positions of scape_hip_report_boot_len; the replicate values of its record set ([series][replicate],
    // f64; series = record * n_groups + group), which columns of them have been written since they were allocated, and
    // what scape_hip_report_boot_quantiles returns per series.  boot_pa_usage: scape_hip_report_boot_usage's record set
    // takes the place of boot_len's in the same buffers (series = kept row * n_groups + group), and so do those of the
    // two-population differences (series = record, or kept row); b_kind (a RepBootKind) says whose it is
    RepLabellings boot{"scape_hip_report_boot_mult", "multiplicities"};
    DevBuf b_mult, b_cell, b_q, b_vals, b_lo, b_hi, b_def;
    int64_t b_first = 0, b_series = 0;
    int32_t b_n_boot = 0, b_groups = 0;
    int32_t b_kind = 0;
    std::vector<uint8_t> b_written;
    // render slots
    DevBuf s_rows[2], s_int[2], s_poff[2], s_pre[2], s_len[2], s_roff[2], s_out[2];
    DevBuf s_nnz[2], s_noff[2];        // Matrix Market blocks: entries per row and their scan
    DevBuf s_lk[2], s_loff[2], s_lskip[2], s_lnarr[2];   // ex_pa_len_mat blocks: per record K, offset into n_arr, skip; n_arr
    DevBuf s_urec[2];                  // ex_pa_usage_mat blocks: per row its record among those of the totals
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
    delete s;                          // every DevBuf frees itself
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

// ---- expected pA length per (record, column) ------------------------------------------------------------------------
// ex_pa_len_mat: the reference's exp_pa_len (apa_core.py:1038-1052) of one cell's reads in one record, from the
// record's K count rows.  For a column with T = sum_l c_l > 0 reads:  v = 1.0 when K == 1, otherwise the sum of
// p_l = (c_l / T) * n_l over l = 0 .. K-1 in the order of numpy's pairwise sum, which np.sum(ws * n_arr) runs (the host
// uploads n_l = 1 + 9 (a_l - a_0) / (a_{K-1} - a_0) as numpy gives it).  Every operation is a correctly rounded IEEE
// one with contraction off, so v is the reference's double bit for bit.  A thread owns a column and keeps T, the eight
// accumulators and the decimal digits in registers.
//
// p_l; a zero count gives (+0) * n_l without the division (0 / T is +0 as well)
__device__ __forceinline__ double rep_len_term(const int32_t *__restrict__ col, int64_t stride,
                                               const double *__restrict__ nn, int l, double T) {
#pragma clang fp contract(off)
    const int32_t c = col[l * stride];
    const double ws = c ? (double)c / T : 0.0;
    return ws * nn[l];
}

// numpy's pairwise sum of p_a .. p_{a+n-1} for n <= 128: sequential from 0.0 below eight terms, otherwise eight
// accumulators over the multiples of eight, their tree, and the remainder one by one
__device__ __forceinline__ double rep_len_leaf(const int32_t *__restrict__ col, int64_t stride,
                                               const double *__restrict__ nn, int a, int n, double T) {
#pragma clang fp contract(off)
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += rep_len_term(col, stride, nn, a + i, T);
        return res;
    }
    double r0 = rep_len_term(col, stride, nn, a, T), r1 = rep_len_term(col, stride, nn, a + 1, T);
    double r2 = rep_len_term(col, stride, nn, a + 2, T), r3 = rep_len_term(col, stride, nn, a + 3, T);
    double r4 = rep_len_term(col, stride, nn, a + 4, T), r5 = rep_len_term(col, stride, nn, a + 5, T);
    double r6 = rep_len_term(col, stride, nn, a + 6, T), r7 = rep_len_term(col, stride, nn, a + 7, T);
    int i = 8;
    for (; i < n - n % 8; i += 8) {
        r0 += rep_len_term(col, stride, nn, a + i, T);
        r1 += rep_len_term(col, stride, nn, a + i + 1, T);
        r2 += rep_len_term(col, stride, nn, a + i + 2, T);
        r3 += rep_len_term(col, stride, nn, a + i + 3, T);
        r4 += rep_len_term(col, stride, nn, a + i + 4, T);
        r5 += rep_len_term(col, stride, nn, a + i + 5, T);
        r6 += rep_len_term(col, stride, nn, a + i + 6, T);
        r7 += rep_len_term(col, stride, nn, a + i + 7, T);
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += rep_len_term(col, stride, nn, a + i, T);
    return res;
}

// Above 128 terms numpy halves: n2 = n / 2 rounded down to a multiple of eight, sum(first n2) + sum(rest), each half the
// same way.  The halves are walked left to right with the open levels on an explicit stack: rest[d] is the length of
// level d's right half, left[d] the finished sum of its left half, bit d of `right` says that the walk is inside the
// right half.  A level at least halves the length, so K < 2^31 opens at most 24 of the 32 levels; the stack is touched
// only when K > 128.  numpy adds the sum to its initial 0.0, which turns a -0.0 into +0.0
#define REP_LEN_LEVELS 32
__device__ __forceinline__ double rep_len_value(const int32_t *__restrict__ col, int64_t stride,
                                                const double *__restrict__ nn, int K, double T) {
#pragma clang fp contract(off)
    if (K == 1) return 1.0;
    if (K <= 128) return 0.0 + rep_len_leaf(col, stride, nn, 0, K, T);
    int rest[REP_LEN_LEVELS];
    double left[REP_LEN_LEVELS];
    uint32_t right = 0;
    int depth = 0, pos = 0, cur = K;
    double v;
    for (;;) {
        while (cur > 128 && depth < REP_LEN_LEVELS) {
            int n2 = cur / 2;
            n2 -= n2 % 8;
            rest[depth] = cur - n2;
            right &= ~(1u << depth);
            ++depth;
            cur = n2;
        }
        v = rep_len_leaf(col, stride, nn, pos, cur > 128 ? 128 : cur, T);   // never above 128 (see the level bound)
        pos += cur;
        while (depth > 0 && ((right >> (depth - 1)) & 1u)) {
            --depth;
            v = left[depth] + v;
        }
        if (depth == 0) break;
        left[depth - 1] = v;
        right |= 1u << (depth - 1);
        cur = rest[depth - 1];
    }
    return 0.0 + v;
}

// Python's '%.6f' % v in integers: v = +-m 2^-s with m < 2^53, x = m 10^6 < 2^73, q = x / 2^s rounded half to even on the
// dropped bits; the text is the sign (of -0.0 and of what rounds to zero as well), the digits of q / 10^6, a point and
// the six digits of q % 10^6.  The caller keeps |v| < 2^31, so s >= 22 and q < 2^51; whatever v is, q fits 64 bits of
// digits and both passes get the same length from it.  Returns q, *neg = the sign bit
__device__ __forceinline__ uint64_t rep_fixed6(double v, int *neg) {
    const uint64_t bits = (uint64_t)__double_as_longlong(v);
    *neg = (int)(bits >> 63);
    const int ex = (int)((bits >> 52) & 0x7ff);
    const uint64_t frac = bits & ((1ull << 52) - 1);
    const uint64_t m = ex ? frac | (1ull << 52) : frac;
    const int s = ex ? 1075 - ex : 1074;
    const unsigned __int128 x = (unsigned __int128)m * 1000000u;
    if (s >= 74) return 0;               // x < 2^73 is less than half of 2^s
    if (s <= 0) return (uint64_t)x;      // |v| >= 2^52, outside the contract
    uint64_t q = (uint64_t)(x >> s);
    const unsigned __int128 rem = x & ((((unsigned __int128)1) << s) - 1), half = ((unsigned __int128)1) << (s - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    return q;
}

__device__ __forceinline__ int rep_fixed6_len(uint64_t q, int neg) { return neg + rep_digits64(q / 1000000u) + 7; }

__device__ __forceinline__ void rep_fixed6_put(char *f, uint64_t q, int neg, int len) {
    uint32_t fr = (uint32_t)(q % 1000000u);
    uint64_t ip = q / 1000000u;
    for (int d = 1; d <= 6; ++d) {
        f[len - d] = (char)('0' + fr % 10);
        fr /= 10;
    }
    f[len - 7] = '.';
    for (int d = len - 8; d >= neg; --d) {
        f[d] = (char)('0' + ip % 10);
        ip /= 10;
    }
    if (neg) f[0] = '-';
}

// one column of record i: T = its reads with label < K (0: no entry) and, for the value text (what == 0), q and the sign
// of the expected pA length; returns the bytes of the entry's last field
__device__ __forceinline__ int rep_len_field(const int32_t *__restrict__ col, int64_t stride,
                                             const double *__restrict__ nn, int K, int what, uint32_t *T_out,
                                             uint64_t *q_out, int *neg_out) {
    uint32_t T = 0;
    for (int l = 0; l < K; ++l) T += (uint32_t)col[l * stride];
    *T_out = T;
    *q_out = 0;
    *neg_out = 0;
    if (!T) return 0;
    if (what) return rep_digits(T);
    *q_out = rep_fixed6(rep_len_value(col, stride, nn, K, (double)T), neg_out);
    return rep_fixed6_len(*q_out, *neg_out);
}

// record i of a block: count rows rec_row0[i] .. + Ks[i] of the last counts call, n_l at n_arr + n_off[i], number
// row_no0 + i of the file; skip[i] != 0 gives it no entry.  Its entries are "<row number> <column + 1> <field>\n" for the
// columns with T > 0, ascending; the field is the value text (what == 0) or T (what == 1).  rnnz[i] = entries,
// rlen[i] = bytes.  Thread t takes the columns t, t + 256, ...: a workgroup reads 256 neighbouring counts of a row at a time
__global__ __launch_bounds__(REP_THREADS) void k_rep_len_mtx_rowlen(const int64_t *__restrict__ rec_row0,
                                                                    const int32_t *__restrict__ Ks,
                                                                    const int64_t *__restrict__ n_off,
                                                                    const double *__restrict__ n_arr,
                                                                    const int8_t *__restrict__ skip, int64_t row_no0,
                                                                    int32_t what, int32_t n_cols,
                                                                    const int32_t *__restrict__ cnt,
                                                                    int64_t *__restrict__ rlen,
                                                                    int64_t *__restrict__ rnnz) {
    __shared__ long long lds[REP_WAVES];
    const int i = blockIdx.x;
    long long n = 0, e = 0;
    if (!skip[i]) {
        const int K = Ks[i];
        const int32_t *rec = cnt + rec_row0[i] * n_cols;
        const double *nn = n_arr + n_off[i];
        for (int c = threadIdx.x; c < n_cols; c += REP_THREADS) {
            uint32_t T;
            uint64_t q;
            int neg;
            const int fd = rep_len_field(rec + c, n_cols, nn, K, what, &T, &q, &neg);
            if (T) {
                ++n;
                e += rep_digits((uint32_t)c + 1) + fd;
            }
        }
    }
    n = rep_block_sum<long long, REP_WAVES>(n, lds);
    e = rep_block_sum<long long, REP_WAVES>(e, lds);
    if (threadIdx.x == 0) {
        rnnz[i] = n;
        rlen[i] = e + n * (rep_digits64((uint64_t)(row_no0 + i)) + 3);   // two spaces and the newline
    }
}

// one workgroup per record, 256 columns per step, as k_rep_mtx_render: each lane's entry position is the tile's running
// offset plus the exclusive scan of the entry lengths (0 for a column without reads below K)
__global__ __launch_bounds__(REP_THREADS) void k_rep_len_mtx_render(const int64_t *__restrict__ rec_row0,
                                                                    const int32_t *__restrict__ Ks,
                                                                    const int64_t *__restrict__ n_off,
                                                                    const double *__restrict__ n_arr,
                                                                    const int8_t *__restrict__ skip, int64_t row_no0,
                                                                    int32_t what, int32_t n_cols,
                                                                    const int32_t *__restrict__ cnt,
                                                                    const int64_t *__restrict__ roff,
                                                                    char *__restrict__ out) {
    __shared__ int lds[REP_WAVES];
    __shared__ char row_txt[20];
    const int i = blockIdx.x;
    if (skip[i] || roff[i + 1] == roff[i]) return;   // the same for every thread of the workgroup
    const int K = Ks[i];
    const int32_t *rec = cnt + rec_row0[i] * n_cols;
    const double *nn = n_arr + n_off[i];
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
        uint32_t T = 0;
        uint64_t q = 0;
        int neg = 0, fd = 0;
        if (c < n_cols) fd = rep_len_field(rec + c, n_cols, nn, K, what, &T, &q, &neg);
        const int cd = T ? rep_digits((uint32_t)c + 1) : 0;
        const int elen = T ? rd + cd + fd + 3 : 0;
        int tile;
        const int ex = rep_block_excl<int, REP_WAVES>(elen, lds, &tile);
        if (T) {
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
            if (what) {
                x = T;
                for (int d = fd - 1; d >= 0; --d) {
                    f[d] = (char)('0' + x % 10);
                    x /= 10;
                }
            } else {
                rep_fixed6_put(f, q, neg, fd);
            }
            f[fd] = '\n';
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
    if (total) HIPCHK(hipMemcpyAsync(s->host_out[slot], s->s_out[slot].p, total, hipMemcpyDeviceToHost, c->stream));
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
    s->u_n_rec = 0;                      // the totals of usage_mat.inc belonged to the counts before
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

int scape_hip_report_render_len_mtx(scape_hip_ctx *c, int32_t slot, int32_t n_rec, const int64_t *rec_row0,
                                    const int32_t *K, const int64_t *n_off, const double *n_arr, const int8_t *skip,
                                    int64_t row_no0, int32_t what, int64_t *bytes_out, int64_t *nnz_out) {
    CTX_ENTER(c);
    ReportState *s = c->rep;
    if (!s || !s->n_cnt_rows) return fail("scape_hip_report_counts has not been called");
    if (slot < 0 || slot > 1 || n_rec <= 0 || !rec_row0 || !K || !n_off || !n_arr || !skip || !bytes_out || !nnz_out)
        return fail("bad argument");
    if (what < 0 || what > 1) return fail("what must be 0 (value) or 1 (reads)");
    if (row_no0 < 1 || row_no0 > INT64_MAX - n_rec) return fail("row_no0 out of range");
    int64_t n_vals = 1;                  // doubles of n_arr that the records name
    for (int i = 0; i < n_rec; ++i) {
        if (K[i] < 1 || rec_row0[i] < 0 || rec_row0[i] > s->n_cnt_rows - K[i]) return fail("record rows out of range");
        if (skip[i]) continue;
        if (n_off[i] < 0 || n_off[i] > INT64_MAX / 16 - K[i]) return fail("n_off out of range");
        n_vals = std::max(n_vals, n_off[i] + K[i]);
    }
    if (s->pending[slot]) {              // the host buffer of this slot is handed over again
        HIPCHK(hipEventSynchronize(s->done[slot]));
        s->pending[slot] = false;
    }
    const int64_t n = n_rec;
    if (s->s_rows[slot].ensure(n * 8) || s->s_len[slot].ensure(n * 8) || s->s_roff[slot].ensure((n + 1) * 8) ||
        s->s_nnz[slot].ensure(n * 8) || s->s_noff[slot].ensure((n + 1) * 8) || s->s_lk[slot].ensure(n * 4) ||
        s->s_loff[slot].ensure(n * 8) || s->s_lskip[slot].ensure(n) || s->s_lnarr[slot].ensure(n_vals * 8))
        return 1;
    HIPCHK(hipMemcpyAsync(s->s_rows[slot].p, rec_row0, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->s_lk[slot].p, K, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->s_loff[slot].p, n_off, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->s_lskip[slot].p, skip, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->s_lnarr[slot].p, n_arr, n_vals * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_rep_len_mtx_rowlen, dim3(n_rec), dim3(REP_THREADS), 0, c->stream,
                       s->s_rows[slot].as<int64_t>(), s->s_lk[slot].as<int32_t>(), s->s_loff[slot].as<int64_t>(),
                       s->s_lnarr[slot].as<double>(), s->s_lskip[slot].as<int8_t>(), row_no0, what, s->n_cols,
                       s->r_cnt.as<int32_t>(), s->s_len[slot].as<int64_t>(), s->s_nnz[slot].as<int64_t>());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rep_scan, dim3(1), dim3(REP_SCAN_THREADS), 0, c->stream, s->s_len[slot].as<int64_t>(), n_rec,
                       s->s_roff[slot].as<int64_t>());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rep_scan, dim3(1), dim3(REP_SCAN_THREADS), 0, c->stream, s->s_nnz[slot].as<int64_t>(), n_rec,
                       s->s_noff[slot].as<int64_t>());
    HIPCHK(hipGetLastError());
    int64_t total = 0, nnz = 0;
    HIPCHK(hipMemcpyAsync(&total, s->s_roff[slot].as<int64_t>() + n_rec, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&nnz, s->s_noff[slot].as<int64_t>() + n_rec, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (total < 0) return fail("negative render block size");
    if (rep_slot_out(s, slot, std::max<int64_t>(total, 1))) return 1;
    if (total) {
        hipLaunchKernelGGL(k_rep_len_mtx_render, dim3(n_rec), dim3(REP_THREADS), 0, c->stream,
                           s->s_rows[slot].as<int64_t>(), s->s_lk[slot].as<int32_t>(), s->s_loff[slot].as<int64_t>(),
                           s->s_lnarr[slot].as<double>(), s->s_lskip[slot].as<int8_t>(), row_no0, what, s->n_cols,
                           s->r_cnt.as<int32_t>(), s->s_roff[slot].as<int64_t>(), s->s_out[slot].as<char>());
        HIPCHK(hipGetLastError());
    }
    if (rep_slot_queue(c, s, slot, total)) return 1;   // a block without an entry is fetched as 0 bytes
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
