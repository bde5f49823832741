// report.inc - the count matrix of merge_pa's output on the device and the reporting stages that read it (included at
// the end of scape_hip.hip, before report_mtx.inc, which renders the same counts as Matrix Market entries, and perm.inc,
// which holds the permutation tests on them).
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
//                   while the device renders block b + 1; the slots and k_rep_scan serve report_mtx.inc as well
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
    // ex_pa_usage_mat (report_mtx.inc): per record of the last scape_hip_report_usage_totals call and column, the reads
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
    DevBuf s_nnz[2], s_noff[2];        // report_mtx.inc's blocks: entries per row and their scan
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

// the nd decimal digits of x at f, back to front
template <typename U>
__device__ __forceinline__ void rep_put_uint(char *f, U x, int nd) {
    for (int d = nd - 1; d >= 0; --d) {
        f[d] = (char)('0' + x % 10);
        x /= 10;
    }
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
                rep_put_uint(f + 2, (uint32_t)v, nd);
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

// a render call takes a slot over: its pinned host buffer is handed over again once the copy queued into it has run
static int rep_slot_claim(ReportState *s, int32_t slot) {
    if (s->pending[slot]) {
        HIPCHK(hipEventSynchronize(s->done[slot]));
        s->pending[slot] = false;
    }
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
    s->u_n_rec = 0;                      // the totals of report_mtx.inc belonged to the counts before
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
    if (rep_slot_claim(s, slot)) return 1;
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
