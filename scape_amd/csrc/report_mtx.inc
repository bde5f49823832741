// report_mtx.inc - every Matrix Market text of the report side: the entries "<row number> <column + 1> <field>\n" of
// ex_pa_cnt_mat --format mtx, ex_pa_len_mat and ex_pa_usage_mat, from the counts of the last scape_hip_report_counts
// call (included from scape_hip.hip directly after report.inc, whose block helpers, rep_digits*, render slots and scan
// it uses).
//
//   k_rep_entries_rowlen<Rule> / k_rep_scan / k_rep_entries_render<Rule>
//                             per row of a block its entries and bytes, their scans, and the entries, through the two
//                             slots.  One walk over the columns per pass; what a column's field is comes from a field
//                             rule, chosen at compile time (k_rep_len_mtx_render, the length matrix's render pass, and
//                             k_rep_usage_mtx_rowlen, the usage matrix's length pass, are the same walk as kernels of
//                             their own: each lost time as an instance of the template):
//       RepCountRule          ex_pa_cnt_mat --format mtx: the count where it is not zero
//       RepLenRule            ex_pa_len_mat: per record and column with T > 0 reads of label < K, '%.6f' of the expected
//                             pA length (what == 0) or T (what == 1)
//       RepUsageRule          ex_pa_usage_mat: '%.6f' of c / T where c > 0 and T >= min_reads (what == 0), or T at every
//                             column of the row's record with T >= min_reads, the row's own count zero or not
//                             (what == 1)
//   k_rep_usage_totals        tot[record][column] = the column's reads with label < K in the record, once per record
// A usage row's entries need its record's T in every column: the totals are formed once per record, so the work of a
// record of K sites is 2 K x columns loads (its counts once for the totals, once for its rows) and not K^2 x columns.

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

// ---- pA site usage per (row, column) --------------------------------------------------------------------------------
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

// ---- the field rules ------------------------------------------------------------------------------------------------
// A rule is passed to the two kernels by value and holds what the host sets: `rows` (the first count row of every row
// of the block; the host frame sets it), the matrix's other per-row arrays and its scalars.
//   open(i, cnt, n_cols, &r)  binds r, the rule's Row, to row i of the block; false: the row has no entry (it is not
//                             walked)
//   r.has(c, &x)              whether column c has an entry; x takes what len() and put() need
//   r.len(x)                  the bytes of that entry's field
//   r.put(f, x, fd)           the field's fd bytes at f
// The presence test stands apart from the length so that the walk branches once per column: a length that means
// "no entry" when it is 0 cost the count matrix's length pass a second divergent region per column.  `what`, where a
// rule has it, is the same for every thread of a launch.
//
// count row rows[i]: an entry where the count is not zero, the field is the count
struct RepCountRule {
    const int64_t *rows;
    struct Field {
        uint32_t v;
    };
    struct Row {
        const int32_t *row;
        __device__ __forceinline__ bool has(int c, Field *x) const {
            x->v = (uint32_t)row[c];
            return x->v != 0;
        }
        __device__ __forceinline__ int len(const Field &x) const { return rep_digits(x.v); }
        __device__ __forceinline__ void put(char *f, const Field &x, int fd) const { rep_put_uint(f, x.v, fd); }
    };
    __device__ __forceinline__ bool open(int i, const int32_t *cnt, int32_t n_cols, Row *r) const {
        r->row = cnt + rows[i] * n_cols;
        return true;
    }
};

// record i: count rows rows[i] .. + Ks[i], n_l at n_arr + n_off[i]; skip[i] != 0 gives it no entry.  An entry where
// T > 0; the field is the value text (what == 0) or T (what == 1).  Thread t takes the columns t, t + 256, ...: a
// workgroup reads 256 neighbouring counts of a row at a time.  The rule serves the length pass only and its Row has no
// put(): the render pass is k_rep_len_mtx_render below
struct RepLenRule {
    const int64_t *rows;
    const int32_t *Ks;
    const int64_t *n_off;
    const double *n_arr;
    const int8_t *skip;
    int32_t what;
    struct Field {
        uint32_t T;
        uint64_t q;
        int neg, fd;
    };
    struct Row {
        const int32_t *rec;
        const double *nn;
        int64_t stride;
        int K, what;
        __device__ __forceinline__ bool has(int c, Field *x) const {
            x->fd = rep_len_field(rec + c, stride, nn, K, what, &x->T, &x->q, &x->neg);
            return x->T != 0;
        }
        __device__ __forceinline__ int len(const Field &x) const { return x.fd; }
    };
    __device__ __forceinline__ bool open(int i, const int32_t *cnt, int32_t n_cols, Row *r) const {
        if (skip[i]) return false;
        r->K = Ks[i];
        r->what = what;
        r->rec = cnt + rows[i] * n_cols;
        r->nn = n_arr + n_off[i];
        r->stride = n_cols;
        return true;
    }
};

// count row rows[i], totals row row_rec[i] of the last totals call: the value text where c > 0 and T >= min_reads
// (what == 0), or T where T >= min_reads (what == 1).  The division is put()'s: the value's bytes are known without it
struct RepUsageRule {
    const int64_t *rows;
    const int32_t *row_rec;
    const int32_t *tot;
    uint32_t min_reads;
    int32_t what;
    struct Field {
        int32_t v;
        uint32_t T;
        int fd;
    };
    struct Row {
        const int32_t *row, *trow;
        uint32_t min_reads;
        int what;
        __device__ __forceinline__ bool has(int c, Field *x) const {
            x->v = row[c];
            x->T = (uint32_t)trow[c];
            x->fd = rep_usage_field_len(x->v, x->T, min_reads, what);
            return x->fd != 0;
        }
        __device__ __forceinline__ int len(const Field &x) const { return x.fd; }
        __device__ __forceinline__ void put(char *f, const Field &x, int fd) const {
            if (what)
                rep_put_uint(f, x.T, fd);
            else
                rep_fixed6_put(f, rep_usage_q(x.v, x.T), 0, fd);
        }
    };
    __device__ __forceinline__ bool open(int i, const int32_t *cnt, int32_t n_cols, Row *r) const {
        r->row = cnt + rows[i] * n_cols;
        r->trow = tot + (int64_t)row_rec[i] * n_cols;
        r->min_reads = min_reads;
        r->what = what;
        return true;
    }
};

// ---- the entry walk -------------------------------------------------------------------------------------------------
// the row number's digits into LDS, once per workgroup; returns their number.  Ends in a barrier
__device__ __forceinline__ int rep_row_text(char *row_txt, uint64_t row_no) {
    const int rd = rep_digits64(row_no);
    if (threadIdx.x == 0) rep_put_uint(row_txt, row_no, rd);
    __syncthreads();
    return rd;
}

// "<row number> <column + 1> " at f and the newline behind the fd bytes of the field; returns where the field goes
__device__ __forceinline__ char *rep_put_entry(char *f, const char *row_txt, int rd, int c, int cd, int fd) {
    for (int d = 0; d < rd; ++d) f[d] = row_txt[d];
    f[rd] = ' ';
    f += rd + 1;
    rep_put_uint(f, (uint32_t)c + 1, cd);
    f[cd] = ' ';
    f += cd + 1;
    f[fd] = '\n';
    return f;
}

// row i of a block has the number row_no0 + i of the file; its entries are "<row number> <column + 1> <field>\n" for
// the columns that the rule gives a field, ascending.  rnnz[i] = entries, rlen[i] = bytes
template <typename Rule>
__global__ __launch_bounds__(REP_THREADS) void k_rep_entries_rowlen(const Rule rule, int64_t row_no0, int32_t n_cols,
                                                                    const int32_t *__restrict__ cnt,
                                                                    int64_t *__restrict__ rlen,
                                                                    int64_t *__restrict__ rnnz) {
    __shared__ long long lds[REP_WAVES];
    const int i = blockIdx.x;
    long long n = 0, e = 0;
    typename Rule::Row row;
    if (rule.open(i, cnt, n_cols, &row)) {
        for (int c = threadIdx.x; c < n_cols; c += REP_THREADS) {
            typename Rule::Field x;
            if (row.has(c, &x)) {
                ++n;
                e += rep_digits((uint32_t)c + 1) + row.len(x);
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

// one workgroup per row, 256 columns per step: each lane's entry position is the tile's running offset plus the
// exclusive scan of the entry lengths (0 for a column without an entry); the row number is formatted once, into LDS.  A
// row without bytes, one that open() refuses among them, is left before the barrier
template <typename Rule>
__global__ __launch_bounds__(REP_THREADS) void k_rep_entries_render(const Rule rule, int64_t row_no0, int32_t n_cols,
                                                                    const int32_t *__restrict__ cnt,
                                                                    const int64_t *__restrict__ roff,
                                                                    char *__restrict__ out) {
    __shared__ int lds[REP_WAVES];
    __shared__ char row_txt[20];
    const int i = blockIdx.x;
    if (roff[i + 1] == roff[i]) return;  // the same for every thread of the workgroup
    typename Rule::Row row;
    rule.open(i, cnt, n_cols, &row);
    const int rd = rep_row_text(row_txt, (uint64_t)(row_no0 + i));
    char *dst = out + roff[i];
    int64_t pos = 0;
    for (int base = 0; base < n_cols; base += REP_THREADS) {
        const int c = base + threadIdx.x;
        typename Rule::Field x;
        // a lane beyond the last column looks at the last one and drops it: the loads stay outside a divergent region
        const bool on = row.has(c < n_cols ? c : n_cols - 1, &x) && c < n_cols;
        const int fd = on ? row.len(x) : 0;
        const int cd = on ? rep_digits((uint32_t)c + 1) : 0;
        const int elen = on ? rd + cd + fd + 3 : 0;
        int tile;
        const int ex = rep_block_excl<int, REP_WAVES>(elen, lds, &tile);
        if (on) row.put(rep_put_entry(dst + pos + ex, row_txt, rd, c, cd, fd), x, fd);
        pos += tile;
    }
}

// The length matrix's render pass is the same walk as a kernel of its own because every pointer is a __restrict__
// argument here: with the pointers coming out of the rule the compiler needs 120 VGPRs for it against 108
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
    const int rd = rep_row_text(row_txt, (uint64_t)(row_no0 + i));
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
            char *f = rep_put_entry(dst + pos + ex, row_txt, rd, c, cd, fd);
            if (what)
                rep_put_uint(f, T, fd);
            else
                rep_fixed6_put(f, q, neg, fd);
        }
        pos += tile;
    }
}

// The usage matrix's length pass is a kernel of its own as well: as k_rep_entries_rowlen<RepUsageRule> its column loop
// is the same instructions, yet its value text measured 0.8 % above this kernel's (profiles/mtx_one_walk_timing.txt)
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

// ---- host side ------------------------------------------------------------------------------------------------------
// the two passes of a rule: the shared walk, or the kernel that stands for it
template <typename Rule>
static void rep_launch_rowlen(const Rule &rule, int32_t n_rows, hipStream_t stream, int64_t row_no0, int32_t n_cols,
                              const int32_t *cnt, int64_t *rlen, int64_t *rnnz) {
    hipLaunchKernelGGL(k_rep_entries_rowlen<Rule>, dim3(n_rows), dim3(REP_THREADS), 0, stream, rule, row_no0, n_cols, cnt,
                       rlen, rnnz);
}

static void rep_launch_rowlen(const RepUsageRule &rule, int32_t n_rows, hipStream_t stream, int64_t row_no0,
                              int32_t n_cols, const int32_t *cnt, int64_t *rlen, int64_t *rnnz) {
    hipLaunchKernelGGL(k_rep_usage_mtx_rowlen, dim3(n_rows), dim3(REP_THREADS), 0, stream, rule.rows, rule.row_rec,
                       row_no0, rule.min_reads, rule.what, n_cols, cnt, rule.tot, rlen, rnnz);
}

template <typename Rule>
static void rep_launch_render(const Rule &rule, int32_t n_rows, hipStream_t stream, int64_t row_no0, int32_t n_cols,
                              const int32_t *cnt, const int64_t *roff, char *out) {
    hipLaunchKernelGGL(k_rep_entries_render<Rule>, dim3(n_rows), dim3(REP_THREADS), 0, stream, rule, row_no0, n_cols, cnt,
                       roff, out);
}

static void rep_launch_render(const RepLenRule &rule, int32_t n_rows, hipStream_t stream, int64_t row_no0,
                              int32_t n_cols, const int32_t *cnt, const int64_t *roff, char *out) {
    hipLaunchKernelGGL(k_rep_len_mtx_render, dim3(n_rows), dim3(REP_THREADS), 0, stream, rule.rows, rule.Ks, rule.n_off,
                       rule.n_arr, rule.skip, row_no0, rule.what, n_cols, cnt, roff, out);
}

// One block of n rows into a slot: the rule's rows uploaded, entries and bytes per row, their scans, the text, and the
// copy to the host queued.  rule.rows is set here; what else the rule points to has been uploaded by the caller.  A
// block without an entry is an error, or with empty_ok is fetched as 0 bytes
template <typename Rule>
static int rep_render_entries(scape_hip_ctx *c, ReportState *s, int32_t slot, int32_t n_rows, const int64_t *rows,
                              Rule rule, int64_t row_no0, bool empty_ok, int64_t *bytes_out, int64_t *nnz_out) {
    const int64_t n = n_rows;
    if (s->s_rows[slot].ensure(n * 8) || s->s_len[slot].ensure(n * 8) || s->s_roff[slot].ensure((n + 1) * 8) ||
        s->s_nnz[slot].ensure(n * 8) || s->s_noff[slot].ensure((n + 1) * 8))
        return 1;
    HIPCHK(hipMemcpyAsync(s->s_rows[slot].p, rows, n * 8, hipMemcpyHostToDevice, c->stream));
    rule.rows = s->s_rows[slot].as<int64_t>();
    rep_launch_rowlen(rule, n_rows, c->stream, row_no0, s->n_cols, s->r_cnt.as<int32_t>(), s->s_len[slot].as<int64_t>(),
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
    if (!empty_ok && total <= 0) return fail("empty render block");
    if (total < 0) return fail("negative render block size");
    if (rep_slot_out(s, slot, std::max<int64_t>(total, 1))) return 1;
    if (total) {
        rep_launch_render(rule, n_rows, c->stream, row_no0, s->n_cols, s->r_cnt.as<int32_t>(),
                          s->s_roff[slot].as<int64_t>(), s->s_out[slot].as<char>());
        HIPCHK(hipGetLastError());
    }
    if (rep_slot_queue(c, s, slot, total)) return 1;
    *bytes_out = total;
    *nnz_out = nnz;
    return 0;
}

extern "C" {

int scape_hip_report_render_mtx(scape_hip_ctx *c, int32_t slot, int32_t n_rows, const int64_t *rows, int64_t row_no0,
                                int64_t *bytes_out, int64_t *nnz_out) {
    CTX_ENTER(c);
    ReportState *s = c->rep;
    if (!s || !s->n_cnt_rows) return fail("scape_hip_report_counts has not been called");
    if (slot < 0 || slot > 1 || n_rows <= 0 || !rows || !bytes_out || !nnz_out) return fail("bad argument");
    if (row_no0 < 1 || row_no0 > INT64_MAX - n_rows) return fail("row_no0 out of range");
    for (int i = 0; i < n_rows; ++i)
        if (rows[i] < 0 || rows[i] >= s->n_cnt_rows) return fail("row index out of range");
    if (rep_slot_claim(s, slot)) return 1;
    return rep_render_entries(c, s, slot, n_rows, rows, RepCountRule{}, row_no0, false, bytes_out, nnz_out);
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
    if (rep_slot_claim(s, slot)) return 1;
    const int64_t n = n_rec;
    if (s->s_lk[slot].ensure(n * 4) || s->s_loff[slot].ensure(n * 8) || s->s_lskip[slot].ensure(n) ||
        s->s_lnarr[slot].ensure(n_vals * 8))
        return 1;
    HIPCHK(hipMemcpyAsync(s->s_lk[slot].p, K, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->s_loff[slot].p, n_off, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->s_lskip[slot].p, skip, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->s_lnarr[slot].p, n_arr, n_vals * 8, hipMemcpyHostToDevice, c->stream));
    RepLenRule rule{};
    rule.Ks = s->s_lk[slot].as<int32_t>();
    rule.n_off = s->s_loff[slot].as<int64_t>();
    rule.n_arr = s->s_lnarr[slot].as<double>();
    rule.skip = s->s_lskip[slot].as<int8_t>();
    rule.what = what;
    return rep_render_entries(c, s, slot, n_rec, rec_row0, rule, row_no0, true, bytes_out, nnz_out);
}

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
    if (rep_slot_claim(s, slot)) return 1;
    if (s->s_urec[slot].ensure((int64_t)n_rows * 4)) return 1;
    HIPCHK(hipMemcpyAsync(s->s_urec[slot].p, row_rec, (int64_t)n_rows * 4, hipMemcpyHostToDevice, c->stream));
    RepUsageRule rule{};
    rule.row_rec = s->s_urec[slot].as<int32_t>();
    rule.tot = s->u_tot.as<int32_t>();
    rule.min_reads = (uint32_t)min_reads;
    rule.what = what;
    return rep_render_entries(c, s, slot, n_rows, rows, rule, row_no0, true, bytes_out, nnz_out);
}

}  // extern "C"
