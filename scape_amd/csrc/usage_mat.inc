// usage_mat.inc - ex_pa_usage_mat: the per-cell usage (PSI) of every pA site, c_l / T, as Matrix Market entries from
// the counts of the last scape_hip_report_counts call (included from scape_hip.hip directly after report.inc, whose
// block helpers, rep_digits*, rep_fixed6*, render slots and scan it uses).
//
//   k_rep_usage_totals        tot[record][column] = the column's reads with label < K in the record, once per record
//   k_rep_usage_mtx_rowlen / k_rep_scan / k_rep_usage_mtx_render
//                             per kept row its entries and bytes, their scans, and the entries, through the two slots;
//                             `what` picks the value text ('%.6f' of c / T where c > 0) or the reads text (T, at every
//                             column of the record's with T >= min_reads, the row's own count zero or not)
// A row's entries need its record's T in every column: the totals are formed once per record, so the work of a record
// of K sites is 2 K x columns loads (its counts once for the totals, once for its rows) and not K^2 x columns.

// tot[i][c] = sum over l < Ks[i] of cnt[rec_row0[i] + l][c].  blockIdx.x = record, blockIdx.y = column slab: thread t of
// slab y owns the columns 256 y + t, + 256 gridDim.y, ... and walks the K rows, so every load of a wavefront is 64
// neighbouring int32.  A record holds at most INT32_MAX reads: the sum fits
__global__ __launch_bounds__(REP_THREADS) void k_rep_usage_totals(const int64_t *__restrict__ rec_row0,
                                                                  const int32_t *__restrict__ Ks, int32_t n_cols,
                                                                  const int32_t *__restrict__ cnt,
                                                                  int32_t *__restrict__ tot) {
    const int i = blockIdx.x;
    const int K = Ks[i];
    const int32_t *rec = cnt + rec_row0[i] * n_cols;
    int32_t *out = tot + (int64_t)i * n_cols;
    for (int c = blockIdx.y * REP_THREADS + threadIdx.x; c < n_cols; c += gridDim.y * REP_THREADS) {
        uint32_t T = 0;
#pragma unroll 4
        for (int l = 0; l < K; ++l) T += (uint32_t)rec[(int64_t)l * n_cols + c];
        out[c] = (int32_t)T;
    }
}

// one column of a kept row: count c, its record's T.  Returns the bytes of the entry's last field, 0 = no entry.  A
// value's text is always 8 bytes: 0 < c <= T gives 0 < c / T <= 1, rep_fixed6 of it is at most 10^6 and the integer
// part one digit, so the length pass does not divide
#define REP_USAGE_VALUE_BYTES 8
__device__ __forceinline__ int rep_usage_field_len(int32_t c, uint32_t T, uint32_t min_reads, int what) {
    if (T < min_reads) return 0;         // min_reads >= 1: an entry has T > 0
    if (what) return rep_digits(T);
    return c > 0 ? REP_USAGE_VALUE_BYTES : 0;
}

// the value of an entry: rep_fixed6 of the double c / T, one correctly rounded division (the sign is clear)
__device__ __forceinline__ uint64_t rep_usage_q(int32_t c, uint32_t T) {
#pragma clang fp contract(off)
    int neg;
    return rep_fixed6((double)c / (double)T, &neg);
}

// row i of a block: count row rows[i] of the last counts call, totals row row_rec[i] of the last totals call, number
// row_no0 + i of the file.  Its entries are "<row number> <column + 1> <field>\n", columns ascending: the value text where
// c > 0 and T >= min_reads (what == 0), or T where T >= min_reads (what == 1).  rnnz[i] = entries, rlen[i] = bytes
__global__ __launch_bounds__(REP_THREADS) void k_rep_usage_mtx_rowlen(const int64_t *__restrict__ rows,
                                                                      const int32_t *__restrict__ row_rec,
                                                                      int64_t row_no0, uint32_t min_reads, int32_t what,
                                                                      int32_t n_cols, const int32_t *__restrict__ cnt,
                                                                      const int32_t *__restrict__ tot,
                                                                      int64_t *__restrict__ rlen,
                                                                      int64_t *__restrict__ rnnz) {
    __shared__ long long lds[REP_WAVES];
    const int i = blockIdx.x;
    const int32_t *row = cnt + rows[i] * n_cols;
    const int32_t *trow = tot + (int64_t)row_rec[i] * n_cols;
    long long n = 0, e = 0;
    for (int c = threadIdx.x; c < n_cols; c += REP_THREADS) {
        const int fd = rep_usage_field_len(row[c], (uint32_t)trow[c], min_reads, what);
        if (fd) {
            ++n;
            e += rep_digits((uint32_t)c + 1) + fd;
        }
    }
    n = rep_block_sum<long long, REP_WAVES>(n, lds);
    e = rep_block_sum<long long, REP_WAVES>(e, lds);
    if (threadIdx.x == 0) {
        rnnz[i] = n;
        rlen[i] = e + n * (rep_digits64((uint64_t)(row_no0 + i)) + 3);   // two spaces and the newline
    }
}

// one workgroup per row, 256 columns per step, as k_rep_mtx_render: each lane's entry position is the tile's running
// offset plus the exclusive scan of the entry lengths (0 for a column without an entry)
__global__ __launch_bounds__(REP_THREADS) void k_rep_usage_mtx_render(const int64_t *__restrict__ rows,
                                                                      const int32_t *__restrict__ row_rec,
                                                                      int64_t row_no0, uint32_t min_reads, int32_t what,
                                                                      int32_t n_cols, const int32_t *__restrict__ cnt,
                                                                      const int32_t *__restrict__ tot,
                                                                      const int64_t *__restrict__ roff,
                                                                      char *__restrict__ out) {
    __shared__ int lds[REP_WAVES];
    __shared__ char row_txt[20];
    const int i = blockIdx.x;
    if (roff[i + 1] == roff[i]) return;  // the same for every thread of the workgroup
    const int32_t *row = cnt + rows[i] * n_cols;
    const int32_t *trow = tot + (int64_t)row_rec[i] * n_cols;
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
        const int32_t v = c < n_cols ? row[c] : 0;
        const uint32_t T = c < n_cols ? (uint32_t)trow[c] : 0;
        const int fd = rep_usage_field_len(v, T, min_reads, what);   // 0 beyond the last column: T = 0 < min_reads
        const int cd = fd ? rep_digits((uint32_t)c + 1) : 0;
        const int elen = fd ? rd + cd + fd + 3 : 0;
        int tile;
        const int ex = rep_block_excl<int, REP_WAVES>(elen, lds, &tile);
        if (fd) {
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
                rep_fixed6_put(f, rep_usage_q(v, T), 0, fd);
            }
            f[fd] = '\n';
        }
        pos += tile;
    }
}

extern "C" {

int scape_hip_report_usage_totals(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row0, const int32_t *K) {
    CTX_ENTER(c);
    ReportState *s = c->rep;
    if (!s || !s->n_cnt_rows) return fail("scape_hip_report_counts has not been called");
    if (n_rec <= 0 || !rec_row0 || !K) return fail("bad argument");
    for (int i = 0; i < n_rec; ++i)
        if (K[i] < 1 || rec_row0[i] < 0 || rec_row0[i] > s->n_cnt_rows - K[i]) return fail("record rows out of range");
    for (int k = 0; k < 2; ++k)          // a queued render may still read the totals of the call before
        if (s->pending[k]) HIPCHK(hipEventSynchronize(s->done[k]));
    s->u_n_rec = 0;
    const int64_t n = n_rec;
    if (s->u_row0.ensure(n * 8) || s->u_K.ensure(n * 4) || s->u_tot.ensure(n * s->n_cols * 4)) return 1;
    s->u_rows.assign(rec_row0, rec_row0 + n);
    s->u_Ks.assign(K, K + n);
    HIPCHK(hipMemcpyAsync(s->u_row0.p, s->u_rows.data(), n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->u_K.p, s->u_Ks.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    // enough column slabs that a batch of few records still fills the device
    const int32_t slabs = (s->n_cols + REP_THREADS - 1) / REP_THREADS;
    const int32_t gy = std::max(1, std::min(slabs, (1024 + n_rec - 1) / n_rec));
    hipLaunchKernelGGL(k_rep_usage_totals, dim3(n_rec, gy), dim3(REP_THREADS), 0, c->stream, s->u_row0.as<int64_t>(),
                       s->u_K.as<int32_t>(), s->n_cols, s->r_cnt.as<int32_t>(), s->u_tot.as<int32_t>());
    HIPCHK(hipGetLastError());
    s->u_n_rec = n_rec;
    return 0;
}

int scape_hip_report_render_usage_mtx(scape_hip_ctx *c, int32_t slot, int32_t n_rows, const int64_t *rows,
                                      const int32_t *row_rec, int64_t row_no0, int32_t min_reads, int32_t what,
                                      int64_t *bytes_out, int64_t *nnz_out) {
    CTX_ENTER(c);
    ReportState *s = c->rep;
    if (!s || !s->n_cnt_rows) return fail("scape_hip_report_counts has not been called");
    if (!s->u_n_rec) return fail("scape_hip_report_usage_totals has not been called");
    if (slot < 0 || slot > 1 || n_rows <= 0 || !rows || !row_rec || !bytes_out || !nnz_out) return fail("bad argument");
    if (what < 0 || what > 1) return fail("what must be 0 (value) or 1 (reads)");
    if (min_reads < 1) return fail("min_reads must be at least 1");
    if (row_no0 < 1 || row_no0 > INT64_MAX - n_rows) return fail("row_no0 out of range");
    for (int i = 0; i < n_rows; ++i) {
        if (rows[i] < 0 || rows[i] >= s->n_cnt_rows) return fail("row index out of range");
        if (row_rec[i] < 0 || row_rec[i] >= s->u_n_rec) return fail("record index out of range");
        const int64_t l = rows[i] - s->u_rows[row_rec[i]];
        if (l < 0 || l >= s->u_Ks[row_rec[i]]) return fail("a row is not one of its record's");
    }
    if (s->pending[slot]) {              // the host buffer of this slot is handed over again
        HIPCHK(hipEventSynchronize(s->done[slot]));
        s->pending[slot] = false;
    }
    const int64_t n = n_rows;
    if (s->s_rows[slot].ensure(n * 8) || s->s_urec[slot].ensure(n * 4) || s->s_len[slot].ensure(n * 8) ||
        s->s_roff[slot].ensure((n + 1) * 8) || s->s_nnz[slot].ensure(n * 8) || s->s_noff[slot].ensure((n + 1) * 8))
        return 1;
    HIPCHK(hipMemcpyAsync(s->s_rows[slot].p, rows, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->s_urec[slot].p, row_rec, n * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_rep_usage_mtx_rowlen, dim3(n_rows), dim3(REP_THREADS), 0, c->stream,
                       s->s_rows[slot].as<int64_t>(), s->s_urec[slot].as<int32_t>(), row_no0, (uint32_t)min_reads, what,
                       s->n_cols, s->r_cnt.as<int32_t>(), s->u_tot.as<int32_t>(), s->s_len[slot].as<int64_t>(),
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
    if (total < 0) return fail("negative render block size");
    if (rep_slot_out(s, slot, std::max<int64_t>(total, 1))) return 1;
    if (total) {
        hipLaunchKernelGGL(k_rep_usage_mtx_render, dim3(n_rows), dim3(REP_THREADS), 0, c->stream,
                           s->s_rows[slot].as<int64_t>(), s->s_urec[slot].as<int32_t>(), row_no0, (uint32_t)min_reads,
                           what, s->n_cols, s->r_cnt.as<int32_t>(), s->u_tot.as<int32_t>(),
                           s->s_roff[slot].as<int64_t>(), s->s_out[slot].as<char>());
        HIPCHK(hipGetLastError());
    }
    if (rep_slot_queue(c, s, slot, total)) return 1;   // a block without an entry is fetched as 0 bytes
    *bytes_out = total;
    *nnz_out = nnz;
    return 0;
}

}  // extern "C"
