// perm.inc - the permutation tests on merge_pa's count matrix: diff_pa and diff_pa_len (freely or within strata),
// diff_pa_groups, diff_pa_len_groups, diff_pa_pairs, diff_pa_markers, diff_pa_len_pairs, diff_pa_len_markers,
// diff_pa_trend and diff_pa_len_trend (included by
// scape_hip.hip after report.inc, whose ReportState, block helpers and k_rep_scan it uses).
//
// A test is two calls.  The first builds the labellings of a chunk of permutations, in exact integers:
//   rep_select_key  the one radix select of the file: the key of a given rank among the hashed 64-bit keys of a set of
//                   positions, by the whole workgroup
//   k_rep_perm_mask_strata
//                   two populations: the membership bits of every permutation, labels permuted within strata (the free
//                   permutation is the case of one stratum).  One workgroup per permutation; per stratum the m1[s]-th
//                   smallest key of its cells, by one wave for a stratum of up to 256 cells and by rep_select_key for a
//                   larger one
//   k_rep_perm_labels
//                   G = 2..64 populations: one byte per (position, permutation) names the group, from the G - 1 cut
//                   keys that rep_select_key finds; one workgroup per permutation
// The second compacts the kept count rows to their nonzeros and runs the statistic, one lane per permutation:
//   k_rep_perm_rowstat or k_rep_groups_rowstat / k_rep_scan / k_rep_perm_fill
//                   per kept row its nonzeros and its sums per population as observed, their scan, and the (position,
//                   count) pairs (rep_perm_prepare)
//   rep_perm_segsum the one walk over mask words: a run of nonzeros summed over the lane's population 1
//   k_rep_perm_test diff_pa: exceedance counts per site and record
//   k_rep_perm_len  diff_pa_len: the record's mean pA position in the two populations (two f64 sums and two integer sums
//                   per lane), exceedance counts per record
//   rep_groups_walk the one walk over label bytes, four in flight: (group, count) of every nonzero to the caller's LDS adds
//   k_rep_groups_obs / k_rep_perm_groups
//                   diff_pa_groups: the observed statistic, and the test with G sums per row and permutation in LDS
//   k_rep_len_groups_obs / k_rep_perm_len_groups
//                   diff_pa_len_groups: the same for the mean pA position, G pairs of exact integer sums per permutation
//                   in LDS, the groups in slices of at most 32
//   k_rep_perm_pair_masks / k_rep_pair_segidx / k_rep_perm_pairs
//                   diff_pa_pairs: the membership bits of every (pair of populations, permutation), per kept row the
//                   first nonzero of every population's column segment, and diff_pa's test for every pair from the one
//                   compaction, a pair walking the nonzeros of its two segments only
//   k_rep_perm_marker_masks / k_rep_perm_markers
//                   diff_pa_markers: the membership bits of every (marker population, permutation) in the order of the
//                   count matrix's columns, each marker's own local positions found by a search in its ranks, and
//                   diff_pa's test of every marker against all other tested cells from the one compaction
//   k_rep_perm_len_pairs / k_rep_perm_len_markers
//                   diff_pa_len_pairs, diff_pa_len_markers: diff_pa_len's test of every pair and of every marker against
//                   the same bits and the same one compaction, one body (rep_perm_len_item), an item walking its own
//                   rows only and finding min x, span and tol over them
//   k_rep_perm_scores / k_rep_trend_obs / k_rep_perm_trend
//                   diff_pa_trend: the rank of EVERY key of a permutation by LDS buckets, so that position j gets the
//                   score q[rank of key(p, j)] as a halfword; the observed sums per kept row; and the test of the
//                   between-site sum of squares of the score and of every site against the record's other reads, the
//                   sums in registers
//   k_rep_len_trend_obs / k_rep_perm_len_trend
//                   diff_pa_len_trend: on the same scores, the covariance of the pA position and the score over a
//                   record's reads as a 128-bit integer, compared exactly; one walk of the nonzeros, no f64
// The last section is not a test but the cell bootstrap on the same compaction (boot_pa_len, boot_pa_usage and their
// two-population differences boot_pa_len_diff, boot_pa_usage_diff):
//   k_rep_boot_mult / k_rep_boot_len / k_rep_boot_usage / k_rep_boot_len_diff / k_rep_boot_usage_diff / k_rep_boot_select
//                   a Poisson(1) multiplicity per (cell, replicate) as a byte, read off the hash by integer comparisons;
//                   per (record, population, replicate) the mean pA position from two exact integer sums, or per (kept
//                   row, population, replicate) the row's share of the population's reads from two; and per series the
//                   two order statistics of a percentile interval by a radix select over a sign-aware key
//                   (rep_boot_values: the one frame of the four kinds of record set).  The value kernels are wrappers of
//                   two bodies, rep_boot_len_body and rep_boot_usage_body, for series of one population or of two: the
//                   _diff kernels form both populations' sums and store the one difference of the two quotients
// On the host a builder leaves a RepLabellings in ReportState (what it built, for the checks of the tests and of the
// `_get` entry points).  A test fills a RepPermCall, the one frame of its call: rep_perm_prepare checks and compacts from
// it, rep_perm_launch_classes launches a two-population test per LDS class of records, rep_perm_count brings the
// exceedance counters back, rep_perm_ranged is the body that diff_pa_pairs and diff_pa_markers share,
// rep_perm_len_ranged that of diff_pa_len_pairs and diff_pa_len_markers behind the same checks (rep_ranged_ok), and
// rep_trend_prepare the head of the two tests on scores.  No entry point returns with work queued on the stream
// (StreamDrain).  Cluster names, strata files, p-values and their adjustment stay on the host (scape_amd/report.py).

// ---- keys and the radix select ----------------------------------------------------------------------------------------
// The tested columns are the first n columns of the count matrix (population 1, then population 2, ...: the caller's
// id2col puts them there), position j = column j.  Permutation p >= 1 ranks the positions by key(p, j); all arithmetic
// mod 2^64 (scape_hip.h states the scheme):
//   mix = the splitmix64 finaliser,  h(p, j) = mix(mix(seed + G p) + G (j + 1)),  key = (h & ~0xFFFFFF) | j
// Keys are distinct (their low 24 bits are j).
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

// Stratum s owns the positions [a1, a1 + m1) of population 1 and [a2, a2 + m2) of population 2 (desc[s] = a1, m1, a2,
// m2; a2 already counts from n1)
__device__ __forceinline__ int rep_strata_pos(int i, int4 d) { return i < d.y ? d.x + i : d.z + (i - d.y); }

// the position maps of rep_select_key: the positions ranked are pos(i), i = 0 .. pos.size() - 1
struct RepAllCells {          // every position of [0, n)
    int n;
    __device__ __forceinline__ int size() const { return n; }
    __device__ __forceinline__ int operator()(int i) const { return i; }
};
struct RepStratumCells {      // the two ranges of one stratum
    int4 d;
    __device__ __forceinline__ int size() const { return d.y + d.w; }
    __device__ __forceinline__ int operator()(int i) const { return rep_strata_pos(i, d); }
};

struct RepSelectLds {
    __align__(16) int hist[256];
    unsigned long long sel[2];    // prefix of the key looked for, and its rank among the keys with that prefix
    int cnt;                      // keys that share the prefix
};

// The key of rank `rank` among key(base, pos(i)), i = 0 .. pos.size() - 1, at least two of them, for the whole workgroup
// (every thread calls): radix select, most significant byte first, a 256-bin LDS histogram per pass, the keys recomputed
// in every pass.  Wave 0 finds the bin that holds the rank with a scan.  The select stops at the first byte after which
// one candidate is left (m keys need about log256(m) + 1 of the 8 passes), and one more pass finds the key that carries
// the selected prefix.  That key is met by one thread: there the function returns true and sets *key; in every other
// thread it returns false.  The caller stores the key from that thread and publishes it with a barrier of its own.
// No barrier follows the one behind the last bin search: past it every thread holds prefix, rank and count in registers,
// the last pass touches no LDS, wave 0 has read hist before it, so a select that follows may clear hist at once, and
// that select writes sel and cnt only behind two barriers of its own, which no thread passes before it has read them
// here.
template <typename Pos>
__device__ __forceinline__ bool rep_select_key(unsigned long long base, Pos pos, int rank, RepSelectLds *lds,
                                               unsigned long long *key) {
    const int lane = threadIdx.x & 63, m = pos.size();
    int *hist = lds->hist;
    unsigned long long prefix = 0;
    int cnt = m, pass = 0;
    for (; pass < 8 && cnt > 1; ++pass) {
        const int shift = 56 - 8 * pass;
        hist[threadIdx.x] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += REP_THREADS) {
            const unsigned long long k = rep_perm_key(base, pos(i));
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
                lds->sel[0] = prefix | ((unsigned long long)b << shift);
                lds->sel[1] = (unsigned long long)r;
                lds->cnt = in_bin;
            }
        }
        __syncthreads();
        prefix = lds->sel[0];
        rank = (int)lds->sel[1];
        cnt = lds->cnt;
    }
    const int known = 64 - 8 * pass;         // m >= 2, so pass >= 1: the bits above `known` are fixed, one key has them
    bool found = false;
    for (int i = threadIdx.x; i < m; i += REP_THREADS) {
        const unsigned long long k = rep_perm_key(base, pos(i));
        if ((k >> known) == (prefix >> known)) {
            *key = k;
            found = true;
        }
    }
    return found;
}

// ---- two populations: membership bits, labels permuted within strata ------------------------------------------------
// Permutation p >= 1 gives population 1 the m1 cells of every stratum with the smallest key(p, j), j the global
// position; the free permutation of diff_pa without --strata_file is the case of one stratum.  The kernel stores, per
// stratum, the EXCLUSIVE bound of the members' keys: 0 when m1 = 0, 2^64 - 1 when m2 = 0 (j <= 2^24 - 2, so every key
// lies below it), otherwise the m1-th smallest key + 1; the last pass then writes bit j = (key(j) < bound[stratum of
// j]) of bits[(j / 64) * p_count + blockIdx.x], so exactly n1 bits are set.
#define REP_STRATA_WAVE_MAX 256   // a wave ranks a stratum of up to this many cells in registers (4 keys per lane)

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
// with rep_select_key over the stratum's two ranges.  bound = bound of this launch [permutation][stratum].
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_mask_strata(
    int32_t n, int32_t n_strata, int32_t n_wave, const int4 *__restrict__ desc, const int32_t *__restrict__ order,
    const int32_t *__restrict__ strat_of, unsigned long long p_first, int32_t p_count, unsigned long long seed,
    unsigned long long *__restrict__ bound, unsigned long long *__restrict__ bits) {
    __shared__ RepSelectLds lds;
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
        const RepStratumCells cells{desc[s]};
        unsigned long long k;
        if (rep_select_key(base, cells, cells.d.y - 1, &lds, &k)) bound_p[s] = k + 1;
    }
    __syncthreads();                         // this permutation's bounds are stored
    const int n_words = (n + 63) >> 6;
    for (int w = wave; w < n_words; w += REP_WAVES) {
        const int j = w * 64 + lane;
        const unsigned long long m = __ballot(j < n && rep_perm_key(base, j) < bound_p[strat_of[j]]);
        if (lane == 0) bits[(int64_t)w * p_count + blockIdx.x] = m;
    }
}

// ---- diff_pa: the kept rows' nonzeros and the test ------------------------------------------------------------------
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

// the sum of the nonzeros nz[k0 .. k1), at the positions column + shift, over this lane's population 1: the nonzeros are
// wave-uniform, the lane tests its own permutation's bit.  Positions ascend, so a mask word is loaded once for all the
// nonzeros that fall into it.  shift = 0 for a row of diff_pa, diff_pa_len and diff_pa_markers (whose bits lie in column
// order); a pair of diff_pa_pairs moves each of its two column segments to the pair's local positions
__device__ __forceinline__ int rep_perm_segsum(const uint2 *__restrict__ nz, int64_t k0, int64_t k1, int shift,
                                               const unsigned long long *__restrict__ mb, int64_t pstride) {
    int a = 0, cur = -1;
    unsigned long long w = 0;
    for (int64_t k = k0; k < k1; ++k) {
        const uint2 e = nz[k];
        const int pos = __builtin_amdgcn_readfirstlane((int)e.x) + shift, c = __builtin_amdgcn_readfirstlane((int)e.y);
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
        for (int64_t i = row0; i < row1; ++i) A += rep_perm_segsum(nz, noff[i], noff[i + 1], 0, mb, p_count);
    double S = 0.0, S0 = 0.0;
    for (int64_t g0 = row0; g0 < row1; g0 += cap) {
        const int64_t g1 = g0 + cap < row1 ? g0 + cap : row1;
        long long Ag = 0;
        for (int64_t i = g0; i < g1; ++i) {
            const int a = rep_perm_segsum(nz, noff[i], noff[i + 1], 0, mb, p_count);
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
        rep_len_row(rep_perm_segsum(nz, noff[i], noff[i + 1], 0, mb, p_count), ti, wi, &W1, &W2, &A, &B);
        rep_len_row((int)a0[i], ti, wi, &V1, &V2, &A0, &B0);
    }
    const double d = rep_len_delta(W1, W2, A, B), d0 = rep_len_delta(V1, V2, A0, B0);
    const unsigned long long b = __ballot(valid && fabs(d) >= fabs(d0) - tol[r]);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&n_ge[r], __popcll(b));
    if (tile == 0 && threadIdx.x == 0) delta0[r] = d0;
}

// ---- G-way labellings (diff_pa_groups) --------------------------------------------------------------------------------
// G = 2..64 populations of sizes n_0 .. n_{G-1}, n = sum n_g tested columns in front of the count matrix, population 0's
// first.  Permutation p >= 1 ranks the n keys key(p, j) (the key of diff_pa, unchanged) and gives the n_0 smallest to
// group 0, the next n_1 to group 1, ...: with c_h = n_0 + .. + n_{h-1} and cut_h = the key of rank c_h - 1 (the largest
// key of the groups below h), h = 1..G-1, the group of position j is #{h : cut_h < key(p, j)}.  With G = 2, group 0 is
// population 1 of k_rep_perm_mask_strata.
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

// one workgroup per permutation p_first + blockIdx.x: the G - 1 cut keys (rank_of_cut[h] = c_{h+1} - 1, ascending, so
// the cut keys ascend too; rep_select_key over all n positions), then one pass that counts, per position, the cut keys
// below its key (binary search in LDS) and writes that group as the byte labels[j * p_count + blockIdx.x].  A
// workgroup's bytes lie p_count apart: the workgroups of neighbouring permutations fill a cache line between them.
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_labels(int32_t n_groups, const int32_t *__restrict__ rank_of_cut,
                                                                 int32_t n, unsigned long long p_first, int32_t p_count,
                                                                 unsigned long long seed, uint8_t *__restrict__ labels) {
    __shared__ RepSelectLds lds;
    __shared__ unsigned long long cuts[REP_GROUPS_MAX - 1];
    const unsigned long long base = rep_mix(seed + REP_PERM_G * (p_first + blockIdx.x));
    const int n_cuts = n_groups - 1;
    for (int h = 0; h < n_cuts; ++h) {
        unsigned long long k;
        if (rep_select_key(base, RepAllCells{n}, rank_of_cut[h], &lds, &k)) cuts[h] = k;
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
// [seg_off[g], seg_off[g + 1]); wave w takes groups w, w + REP_WAVES, ...), t[i] = their sum, nnz[i] = its nonzeros.
// n_groups <= REP_GROUPS_MAX + 1: diff_pa_markers has a segment of other cells behind its 64 markers at most
__global__ __launch_bounds__(REP_THREADS) void k_rep_groups_rowstat(const int64_t *__restrict__ rows, int32_t n_cols,
                                                                    const int32_t *__restrict__ cnt, int32_t n_groups,
                                                                    const int32_t *__restrict__ seg_off,
                                                                    int64_t *__restrict__ nnz, int64_t *__restrict__ t,
                                                                    int64_t *__restrict__ a0) {
    __shared__ long long sum_g[REP_GROUPS_MAX + 1], nz_g[REP_GROUPS_MAX + 1];
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

// the walk of the G-way tests and of the trend test: add(group, count) for every nonzero nz[k0 .. k1), the group under
// this lane's labelling (lb = the lane's element of position 0, the positions pstride elements apart: a byte per group
// label, a halfword per score of diff_pa_trend).  The nonzeros are wave-uniform.  Four at a time: their labels are
// loaded before the first addition waits for one.  The G-way add() adds into the lane's own column of LDS with atomics
// whose results are not used - one ds_add without a return value in place of a read, an add and a write that would
// wait for each other; no other lane touches the address
template <typename Label, typename Add>
__device__ __forceinline__ void rep_groups_walk(const uint2 *__restrict__ nz, int64_t k0, int64_t k1,
                                                const Label *__restrict__ lb, int64_t pstride, Add add) {
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
        for (int u = 0; u < 4; ++u) add(g[u], c[u]);
    }
    for (; k < k1; ++k) {
        const uint2 e = nz[k];
        const int c = __builtin_amdgcn_readfirstlane((int)e.y);
        add((int)lb[(int64_t)__builtin_amdgcn_readfirstlane((int)e.x) * pstride], c);
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
    rep_groups_walk(nz, noff[row0], noff[row1], lb, p_count,
                    [=](int g, int c) { atomicAdd(&accA[g * REP_THREADS], c); });
    double S = 0.0;
    for (int64_t i = row0; i < row1; ++i) {
        for (int g = 0; g < n_groups; ++g) acca[g * REP_THREADS] = 0;
        rep_groups_walk(nz, noff[i], noff[i + 1], lb, p_count,
                        [=](int g, int c) { atomicAdd(&acca[g * REP_THREADS], c); });
        const long long ti = t[i];
        const double s = rep_groups_site<int32_t>(acca, accA, REP_THREADS, n_groups, ti, T);
        S = S + rep_groups_share(s, ti, T);
        const unsigned long long b = __ballot(valid && s >= s0[i] * REP_PERM_SLACK);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(&site_ge[i], __popcll(b));
    }
    const unsigned long long b = __ballot(valid && S >= stat0[r] * REP_PERM_SLACK);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&gene_ge[r], __popcll(b));
}

// ---- diff_pa_len_groups: mean pA position across the G groups ---------------------------------------------------------
// The labellings are the G-way ones above.  Kept row i of a record carries the INTEGER position q_i, 0 <= q_i <= qspan,
// 2^21 <= qspan = max q_i <= 2^22 (the host scales x_i - min x by a power of two and rounds).  Under a labelling with
// a_ig the sum of row i over group g:
//   A_g = sum_i a_ig (32-bit),  Q_g = sum_i a_ig q_i (64-bit),  T = sum_g A_g < 2^31,  Q = sum_g Q_g <= T qspan < 2^53
// Q and T belong to the record; A_g and Q_g are exact integers whatever the order in which the nonzeros arrive.
//   D   = sum_{g : A_g > 0} A_g (Q_g / A_g - Q / T)^2         (groups in order)  the between-group sum of squares
//   d_g = Q_g / A_g - (Q - Q_g) / (T - A_g),  0 when A_g = 0 or A_g = T          group g against all the others
// Rounding of the code below (contraction off, unit roundoff u = 2^-53, first order in u; every mean lies in 0 .. qspan):
//   * (double) of Q_g, A_g, Q - Q_g, T - A_g, Q and T is exact (all below 2^53): the error does not depend on the
//     number of rows or nonzeros;
//   * m = fl(Q / T) and fl(Q_g / A_g) are each within u qspan of the exact mean and their difference e rounds by at most
//     u qspan more: e is within 3 u qspan of mu_g - mu;
//   * e e is within 2 |e| 3 u qspan + u e^2 of (mu_g - mu)^2 and the product with the exact (double)A_g rounds by u more:
//     the term is within A_g (6 u qspan |e| + 2 u e^2), and over the groups, with |e| <= qspan and sum A_g = T, all terms
//     together are within 8 u T qspan^2;
//   * the first addition (0 + term) is exact, each of the other G - 1 rounds by at most u times a partial sum of positive
//     terms that is at most D <= T qspan^2:  |D - exact| <= (G + 7) u T qspan^2 <= (G + 8) u T qspan^2 =: eD;
//   * each of the two means of d_g is within u qspan and the subtraction rounds by at most u qspan:
//     |d_g - exact| <= 3 u qspan =: ed.
// A permutation is counted when D(p) >= D(0) - tolD, tolD = 2^-40 T qspan^2, and when |d_g(p)| >= |d_g(0)| - told,
// told = 2^-40 qspan; the thresholds' own subtractions round by at most u T qspan^2 and u qspan.  A labelling whose exact
// statistic reaches the observed one is counted whatever the rounding, and one more than twice the band below it never
// is, as long as 2 eD + u T qspan^2 <= tolD and 2 ed + u qspan <= told: (2 G + 17) u <= 145 u for G <= 64, and 7 u,
// against 2^-40 = 8,192 u.  Nothing has to be capped beyond G <= 64, q_i <= 2^22 and T < 2^31, which the entry point checks.
#define REP_LEN_GROUPS_SLICE 32        // groups whose sums are in LDS at once: 12 bytes per lane and group, 96 KiB
#define REP_LEN_GROUPS_MAX_Q (1 << 22)

// one group's term of D and its d_g under a labelling, from the exact integers; m = (double)Q / (double)T of the record.
// The observed labelling and every permutation go through these two functions, with contraction off; every operation is
// a correctly rounded IEEE one, so equal integers give equal doubles
__device__ __forceinline__ double rep_len_groups_term(long long Qg, long long Ag, double m) {
#pragma clang fp contract(off)
    if (Ag == 0) return 0.0;
    const double e = (double)Qg / (double)Ag - m;
    return (double)Ag * (e * e);
}

__device__ __forceinline__ double rep_len_groups_delta(long long Qg, long long Ag, long long Q, long long T) {
#pragma clang fp contract(off)
    if (Ag == 0 || Ag == T) return 0.0;
    return (double)Qg / (double)Ag - (double)(Q - Qg) / (double)(T - Ag);
}

// one workgroup per record: the observed labelling.  qt[2 r], qt[2 r + 1] = Q, T and mean[r] = (double)Q / (double)T,
// formed once for every permutation of the record; d0[r * n_groups + g] = d_g(0) by thread g; stat0[r] = D(0), the
// groups' terms added in order by one thread, as a lane of k_rep_perm_len_groups adds them
__global__ __launch_bounds__(REP_THREADS) void k_rep_len_groups_obs(const int64_t *__restrict__ roff,
                                                                    const int64_t *__restrict__ t,
                                                                    const int64_t *__restrict__ a0, int32_t n_groups,
                                                                    const int32_t *__restrict__ q,
                                                                    long long *__restrict__ qt, double *__restrict__ mean,
                                                                    double *__restrict__ d0, double *__restrict__ stat0) {
#pragma clang fp contract(off)
    __shared__ long long A0[REP_GROUPS_MAX], Q0[REP_GROUPS_MAX];
    __shared__ long long QT[2];
    const int r = blockIdx.x;
    const int64_t row0 = roff[r], row1 = roff[r + 1];
    if (threadIdx.x < n_groups) {
        long long A = 0, Q = 0;
        for (int64_t i = row0; i < row1; ++i) {
            const long long a = a0[i * n_groups + threadIdx.x];
            A += a;
            Q += a * q[i];
        }
        A0[threadIdx.x] = A;
        Q0[threadIdx.x] = Q;
    }
    if (threadIdx.x == REP_THREADS - 1) {
        long long T = 0, Q = 0;
        for (int64_t i = row0; i < row1; ++i) {
            T += t[i];
            Q += t[i] * q[i];
        }
        QT[0] = Q;
        QT[1] = T;
    }
    __syncthreads();
    const long long Q = QT[0], T = QT[1];
    const double m = (double)Q / (double)T;
    if (threadIdx.x < n_groups)
        d0[(int64_t)r * n_groups + threadIdx.x] = rep_len_groups_delta(Q0[threadIdx.x], A0[threadIdx.x], Q, T);
    if (threadIdx.x == 0) {
        double D = 0.0;
        for (int g = 0; g < n_groups; ++g) D = D + rep_len_groups_term(Q0[g], A0[g], m);
        qt[2 * r] = Q;
        qt[2 * r + 1] = T;
        mean[r] = m;
        stat0[r] = D;
    }
}

// workgroup = (record blockIdx.x / n_tiles, tile of 256 permutations), one lane per permutation, as k_rep_perm_groups.
// The groups are taken in slices of `slice` <= REP_LEN_GROUPS_SLICE: LDS holds Q_g(p) as accQ[group][lane] (8 bytes;
// a 16-lane access group covers all 32 banks whatever the groups) and behind them A_g(p) as accA[group][lane]: 12 x
// slice x 256 bytes.  One walk over the record's nonzeros per slice forms both; each lane owns its column and no
// barrier is needed.  D and the counters are additive over the groups, and the terms of D are added in group order in a
// register that lives across the slices, so the result does not depend on the slice size.  Exceedances are counted per
// wave (ballot) and added with one atomic per wave and counter: grp_ge[r * n_groups + g] for |d_g|, rec_ge[r] for D.
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_len_groups(
    const uint8_t *__restrict__ labels, int32_t p_count, int32_t n_tiles, int32_t n_groups, int32_t slice,
    const int64_t *__restrict__ roff, const int64_t *__restrict__ noff, const uint2 *__restrict__ nz,
    const int32_t *__restrict__ q, const long long *__restrict__ qt, const double *__restrict__ mean,
    const double *__restrict__ d0, const double *__restrict__ stat0, const double *__restrict__ tol,
    int32_t *__restrict__ grp_ge, int32_t *__restrict__ rec_ge) {
#pragma clang fp contract(off)
    extern __shared__ unsigned long long rep_accq[];
    const int r = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles;
    const int p = tile * REP_THREADS + threadIdx.x;
    const bool valid = p < p_count;
    const uint8_t *lb = labels + (valid ? p : p_count - 1);
    unsigned long long *accQ = rep_accq + threadIdx.x;
    int32_t *accA = reinterpret_cast<int32_t *>(rep_accq + slice * REP_THREADS) + threadIdx.x;
    const int64_t row0 = roff[r], row1 = roff[r + 1];
    const long long Q = qt[2 * r], T = qt[2 * r + 1];
    const double m = mean[r], tolD = tol[2 * r], told = tol[2 * r + 1];
    double D = 0.0;
    for (int g0 = 0; g0 < n_groups; g0 += slice) {
        const int ng = min(slice, n_groups - g0);
        for (int g = 0; g < ng; ++g) {
            accQ[g * REP_THREADS] = 0;
            accA[g * REP_THREADS] = 0;
        }
        for (int64_t i = row0; i < row1; ++i) {
            const long long qi = q[i];       // wave-uniform, and so is count x qi
            rep_groups_walk(nz, noff[i], noff[i + 1], lb, p_count, [=](int g, int c) {
                if ((unsigned)(g - g0) < (unsigned)ng) {     // a label outside the slice adds nothing
                    atomicAdd(&accA[(g - g0) * REP_THREADS], c);
                    atomicAdd(&accQ[(g - g0) * REP_THREADS], (unsigned long long)(c * qi));
                }
            });
        }
        for (int g = 0; g < ng; ++g) {
            const long long Qg = (long long)accQ[g * REP_THREADS], Ag = accA[g * REP_THREADS];
            D = D + rep_len_groups_term(Qg, Ag, m);
            const double d = rep_len_groups_delta(Qg, Ag, Q, T);
            const unsigned long long b = __ballot(valid && fabs(d) >= fabs(d0[(int64_t)r * n_groups + g0 + g]) - told);
            if ((threadIdx.x & 63) == 0 && b) atomicAdd(&grp_ge[(int64_t)r * n_groups + g0 + g], __popcll(b));
        }
    }
    const unsigned long long b = __ballot(valid && D >= stat0[r] - tolD);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&rec_ge[r], __popcll(b));
}

// ---- diff_pa_pairs: every pair of the G populations, each as diff_pa --------------------------------------------------
// The G populations sit in the column segments seg_off in front of the count matrix, as for the G-way tests.  Pair
// (g, h) is diff_pa of population g against population h: its local positions are 0 .. n_g - 1 for g's columns in
// order and n_g .. n_g + n_h - 1 for h's, permutation p >= 1 gives g the n_g local positions with the smallest
// key(p, local position) - the key, the seed and so the labellings of scape_hip_report_perm_masks(n_g, n_h) - and the
// statistics are rep_perm_row's, rows in order.  The kept rows are compacted ONCE over all n positions; a row without a
// read in the pair has t_i = 0 there, adds exactly 0.0 to S (rep_perm_row) and owns no counter the host reads, so S has
// the bits that scape_hip_report_perm_test forms from the pair's own rows.
struct RepPair {
    int32_t g, h, n_g, n_h;       // the two populations and their cells
    int32_t woff, pad[3];         // first mask word of the pair (the words of all pairs together stay below 2^31)
};

// one workgroup per (permutation p_first + blockIdx.x, pair blockIdx.y): the n_g-th smallest key among the pair's local
// positions, by wave 0 alone for up to REP_STRATA_WAVE_MAX cells (one "stratum" of every cell: position i = cell i) and
// by rep_select_key for more; bound[pair][permutation] = that key + 1; then bit j = (key(j) < bound) of
// bits[(woff + j / 64) * p_count + blockIdx.x], the layout k_rep_perm_test reads.  The branch is uniform over the
// workgroup (it depends on the pair only).
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_pair_masks(const RepPair *__restrict__ pairs,
                                                                     unsigned long long p_first, int32_t p_count,
                                                                     unsigned long long seed, unsigned long long *bound,
                                                                     unsigned long long *__restrict__ bits) {
    __shared__ RepSelectLds lds;
    const RepPair pr = pairs[blockIdx.y];
    const int n = pr.n_g + pr.n_h;
    const unsigned long long base = rep_mix(seed + REP_PERM_G * (p_first + blockIdx.x));
    unsigned long long *bound_p = bound + (int64_t)blockIdx.y * p_count + blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (n <= REP_STRATA_WAVE_MAX) {
        const int4 d = make_int4(0, pr.n_g, pr.n_g, pr.n_h);
        if (wave == 0) {
            if (n <= 64) rep_strata_wave<1>(base, d, lane, bound_p);
            else rep_strata_wave<REP_STRATA_WAVE_MAX / 64>(base, d, lane, bound_p);
        }
    } else {
        unsigned long long k;
        if (rep_select_key(base, RepAllCells{n}, pr.n_g - 1, &lds, &k)) *bound_p = k + 1;
    }
    __syncthreads();                         // this labelling's bound is stored
    const unsigned long long b = *bound_p;
    const int n_words = (n + 63) >> 6;
    for (int w = wave; w < n_words; w += REP_WAVES) {
        const int j = w * 64 + lane;
        const unsigned long long m = __ballot(j < n && rep_perm_key(base, j) < b);
        if (lane == 0) bits[((int64_t)pr.woff + w) * p_count + blockIdx.x] = m;
    }
}

// one thread per (kept row i, g = 0 .. n_groups): seg[i * (n_groups + 1) + g] = the first nonzero of the row at or beyond
// column seg_off[g] (binary search; the row's positions ascend), so the nonzeros of group g are seg[..g] .. seg[..g + 1]
__global__ __launch_bounds__(REP_THREADS) void k_rep_pair_segidx(const int64_t *__restrict__ noff,
                                                                 const uint2 *__restrict__ nz,
                                                                 const int32_t *__restrict__ seg_off, int32_t n_groups,
                                                                 int64_t n_rows, int64_t *__restrict__ seg) {
    const int64_t idx = (int64_t)blockIdx.x * REP_THREADS + threadIdx.x;
    if (idx >= n_rows * (n_groups + 1)) return;
    const int64_t i = idx / (n_groups + 1);
    const uint32_t col = (uint32_t)seg_off[idx % (n_groups + 1)];
    int64_t lo = noff[i], hi = noff[i + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (nz[mid].x < col) lo = mid + 1;
        else hi = mid;
    }
    seg[idx] = lo;
}

// workgroup = (pair pair_first + blockIdx.y, record recs[blockIdx.x / n_tiles], tile of 256 permutations), one lane per
// permutation, as k_rep_perm_test: a_i(p) of the record's rows in LDS as acc[row][lane] (each lane its own column, no
// barrier), a record with more than `cap` rows in groups of cap rows behind one extra walk that forms A(p).  sg[i] =
// the row's G + 1 segment starts, a0[i * n_groups + g] its observed sum over group g: t_i, T and A(0) of the pair come
// from them.  The pair tests the record when two rows or more have a read in it and both populations have reads;
// otherwise the workgroup stores S(0) = 0 and leaves (uniform: the decision reads the record's sums only).  A row with
// t_i = 0 is passed over: its share of S is exactly 0.0.  Counters: site_ge[pair in range][row], gene_ge and
// stat0[pair in range][record], one atomic per wave and counter.
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_pairs(
    const unsigned long long *__restrict__ bits, int32_t p_count, int32_t n_tiles, const int32_t *__restrict__ recs,
    const int64_t *__restrict__ roff, const int64_t *__restrict__ sg, const uint2 *__restrict__ nz,
    const int64_t *__restrict__ a0, int32_t n_groups, const int32_t *__restrict__ seg_off,
    const RepPair *__restrict__ pairs, int64_t n_rows, int32_t n_rec, int32_t cap, int32_t *__restrict__ site_ge,
    int32_t *__restrict__ gene_ge, double *__restrict__ stat0) {
#pragma clang fp contract(off)
    extern __shared__ int32_t rep_acc[];
    const RepPair pr = pairs[blockIdx.y];
    const int g = pr.g, h = pr.h, sh_g = -seg_off[g], sh_h = pr.n_g - seg_off[h];
    const int r = recs[blockIdx.x / n_tiles], tile = blockIdx.x % n_tiles;
    const int64_t out_r = (int64_t)blockIdx.y * n_rec + r;
    const int64_t row0 = roff[r], row1 = roff[r + 1];
    long long T = 0, A0 = 0;
    int with_reads = 0;
    for (int64_t i = row0; i < row1; ++i) {
        const long long ag = a0[i * n_groups + g], ah = a0[i * n_groups + h];
        T += ag + ah;
        A0 += ag;
        with_reads += ag + ah > 0;
    }
    if (with_reads < 2 || A0 == 0 || A0 == T) {
        if (tile == 0 && threadIdx.x == 0) stat0[out_r] = 0.0;
        return;
    }
    const int p = tile * REP_THREADS + threadIdx.x;
    const bool valid = p < p_count;
    const unsigned long long *mb = bits + (int64_t)pr.woff * p_count + (valid ? p : p_count - 1);
    int32_t *acc = rep_acc + threadIdx.x;
    int32_t *site = site_ge + (int64_t)blockIdx.y * n_rows;
    const int stride = n_groups + 1;
    long long A = 0;
    const bool one = row1 - row0 <= cap;
    if (!one)
        for (int64_t i = row0; i < row1; ++i) {
            const int64_t *si = sg + i * stride;
            A += rep_perm_segsum(nz, si[g], si[g + 1], sh_g, mb, p_count) +
                 rep_perm_segsum(nz, si[h], si[h + 1], sh_h, mb, p_count);
        }
    double S = 0.0, S0 = 0.0;
    for (int64_t g0 = row0; g0 < row1; g0 += cap) {
        const int64_t g1 = g0 + cap < row1 ? g0 + cap : row1;
        long long Ag = 0;
        for (int64_t i = g0; i < g1; ++i) {
            const int64_t *si = sg + i * stride;
            const int a = rep_perm_segsum(nz, si[g], si[g + 1], sh_g, mb, p_count) +
                          rep_perm_segsum(nz, si[h], si[h + 1], sh_h, mb, p_count);
            acc[(i - g0) * REP_THREADS] = a;
            Ag += a;
        }
        if (one) A = Ag;
        for (int64_t i = g0; i < g1; ++i) {
            const long long a0i = a0[i * n_groups + g], ti = a0i + a0[i * n_groups + h];
            if (ti == 0) continue;
            double d, d0;
            S = S + rep_perm_row(acc[(i - g0) * REP_THREADS], ti, A, T, &d);
            S0 = S0 + rep_perm_row(a0i, ti, A0, T, &d0);
            const unsigned long long b = __ballot(valid && fabs(d) >= fabs(d0) * REP_PERM_SLACK);
            if ((threadIdx.x & 63) == 0 && b) atomicAdd(&site[i], __popcll(b));
        }
    }
    const unsigned long long b = __ballot(valid && S >= S0 * REP_PERM_SLACK);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&gene_ge[out_r], __popcll(b));
    if (tile == 0 && threadIdx.x == 0) stat0[out_r] = S0;
}

// ---- diff_pa_markers: every marker population against all other tested cells, each as diff_pa ------------------------
// The count matrix is laid out as for the G-way tests: marker 0's columns first, then marker 1's, ..., then a segment of
// "others" (tested cells of no marker; it may be empty), columns ascending within a segment; slot j is that position and
// n the tested cells.  Marker g is diff_pa of its population against the n - n_g other tested cells.  diff_pa would put
// g's columns at the local positions 0 .. n_g - 1 and all others, ascending, at n_g .. n - 1: with rank[j] the rank of
// slot j's column among the n tested columns ascending (it ascends within a segment),
//   local_g(j) = j - seg_off[g]                                           for a slot of g's own segment
//   local_g(j) = n_g + rank[j] - #{cells of g with a smaller rank}         for any other slot,
// the count a lower bound in g's ascending slice of rank.  Permutation p >= 1 gives g the n_g local positions with the
// smallest key(p, local position): key, seed and labellings of scape_hip_report_perm_masks(n_g, n - n_g).  The bits are
// stored in SLOT order, so the test walks the one compaction of a row with shift 0, as k_rep_perm_test does, and t_i,
// the kept rows and T are the same for every marker.
__device__ __forceinline__ int rep_marker_local(int j, int s0, int s1, const int32_t *__restrict__ rank) {
    if (j >= s0 && j < s1) return j - s0;
    const int r = rank[j];
    int lo = s0, hi = s1;                    // lo - s0 = cells of the marker whose rank is smaller
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rank[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    return (s1 - s0) + r - (lo - s0);
}

// one workgroup per (permutation p_first + blockIdx.x, marker blockIdx.y): the n_g-th smallest of the n keys key(p, i),
// i < n, by wave 0 alone for n up to REP_STRATA_WAVE_MAX and by rep_select_key for more, as k_rep_perm_pair_masks;
// bound[marker][permutation] = that key + 1; then bit of slot j = (key(p, local_g(j)) < bound) of
// bits[(marker * n_words + j / 64) * p_count + blockIdx.x].  The marker's slice of rank is read by every lane's search
// and stays in cache; the search is 4.7 ms of the launch's 12.2 ms for 12 markers of 20,000 cells and 9,999 permutations
// (profiles/diff_pa_markers_timing.txt, which also says why no table of local positions is kept).  The branch is
// uniform over the workgroup (n is the launch's).
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_marker_masks(const int32_t *__restrict__ seg_off,
                                                                       const int32_t *__restrict__ rank, int32_t n,
                                                                       unsigned long long p_first, int32_t p_count,
                                                                       unsigned long long seed, unsigned long long *bound,
                                                                       unsigned long long *__restrict__ bits) {
    __shared__ RepSelectLds lds;
    const int s0 = seg_off[blockIdx.y], s1 = seg_off[blockIdx.y + 1], n_g = s1 - s0;
    const unsigned long long base = rep_mix(seed + REP_PERM_G * (p_first + blockIdx.x));
    unsigned long long *bound_p = bound + (int64_t)blockIdx.y * p_count + blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (n <= REP_STRATA_WAVE_MAX) {
        const int4 d = make_int4(0, n_g, n_g, n - n_g);
        if (wave == 0) {
            if (n <= 64) rep_strata_wave<1>(base, d, lane, bound_p);
            else rep_strata_wave<REP_STRATA_WAVE_MAX / 64>(base, d, lane, bound_p);
        }
    } else {
        unsigned long long k;
        if (rep_select_key(base, RepAllCells{n}, n_g - 1, &lds, &k)) *bound_p = k + 1;
    }
    __syncthreads();                         // this labelling's bound is stored
    const unsigned long long b = *bound_p;
    const int n_words = (n + 63) >> 6;
    for (int w = wave; w < n_words; w += REP_WAVES) {
        const int j = w * 64 + lane;
        const unsigned long long m = __ballot(j < n && rep_perm_key(base, rep_marker_local(j, s0, s1, rank)) < b);
        if (lane == 0) bits[((int64_t)blockIdx.y * n_words + w) * p_count + blockIdx.x] = m;
    }
}

// workgroup = (marker marker_first + blockIdx.y, record recs[blockIdx.x / n_tiles], tile of 256 permutations), one lane
// per permutation, as k_rep_perm_test: a_i(p) of the record's rows in LDS as acc[row][lane] (each lane its own column, no
// barrier), a record with more than `cap` rows in groups of cap rows behind one extra walk that forms A(p).  t[i] = the
// row's sum over all n tested cells, a0[i * n_seg + g] its observed sum over segment g.  The marker tests the record when
// two rows or more have a read and both the marker and its rest have reads; otherwise the workgroup stores S(0) = 0 and
// leaves (uniform: the decision reads the record's sums only).  Counters: site_ge[marker in range][row], gene_ge and
// stat0[marker in range][record], one atomic per wave and counter.
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_markers(
    const unsigned long long *__restrict__ bits, int32_t p_count, int32_t n_tiles, int32_t n_words,
    const int32_t *__restrict__ recs, const int64_t *__restrict__ roff, const int64_t *__restrict__ noff,
    const uint2 *__restrict__ nz, const int64_t *__restrict__ t, const int64_t *__restrict__ a0, int32_t n_seg,
    int32_t marker_first, int64_t n_rows, int32_t n_rec, int32_t cap, int32_t *__restrict__ site_ge,
    int32_t *__restrict__ gene_ge, double *__restrict__ stat0) {
#pragma clang fp contract(off)
    extern __shared__ int32_t rep_acc[];
    const int g = marker_first + blockIdx.y;
    const int r = recs[blockIdx.x / n_tiles], tile = blockIdx.x % n_tiles;
    const int64_t out_r = (int64_t)blockIdx.y * n_rec + r;
    const int64_t row0 = roff[r], row1 = roff[r + 1];
    const int64_t *a0g = a0 + g;
    long long T = 0, A0 = 0;
    int with_reads = 0;
    for (int64_t i = row0; i < row1; ++i) {
        T += t[i];
        A0 += a0g[i * n_seg];
        with_reads += t[i] > 0;
    }
    if (with_reads < 2 || A0 == 0 || A0 == T) {
        if (tile == 0 && threadIdx.x == 0) stat0[out_r] = 0.0;
        return;
    }
    const int p = tile * REP_THREADS + threadIdx.x;
    const bool valid = p < p_count;
    const unsigned long long *mb = bits + (int64_t)g * n_words * p_count + (valid ? p : p_count - 1);
    int32_t *acc = rep_acc + threadIdx.x;
    int32_t *site = site_ge + (int64_t)blockIdx.y * n_rows;
    long long A = 0;
    const bool one = row1 - row0 <= cap;
    if (!one)
        for (int64_t i = row0; i < row1; ++i) A += rep_perm_segsum(nz, noff[i], noff[i + 1], 0, mb, p_count);
    double S = 0.0, S0 = 0.0;
    for (int64_t g0 = row0; g0 < row1; g0 += cap) {
        const int64_t g1 = g0 + cap < row1 ? g0 + cap : row1;
        long long Ag = 0;
        for (int64_t i = g0; i < g1; ++i) {
            const int a = rep_perm_segsum(nz, noff[i], noff[i + 1], 0, mb, p_count);
            acc[(i - g0) * REP_THREADS] = a;
            Ag += a;
        }
        if (one) A = Ag;
        for (int64_t i = g0; i < g1; ++i) {
            double d, d0;
            S = S + rep_perm_row(acc[(i - g0) * REP_THREADS], t[i], A, T, &d);
            S0 = S0 + rep_perm_row(a0g[i * n_seg], t[i], A0, T, &d0);
            const unsigned long long b = __ballot(valid && fabs(d) >= fabs(d0) * REP_PERM_SLACK);
            if ((threadIdx.x & 63) == 0 && b) atomicAdd(&site[i], __popcll(b));
        }
    }
    const unsigned long long b = __ballot(valid && S >= S0 * REP_PERM_SLACK);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&gene_ge[out_r], __popcll(b));
    if (tile == 0 && threadIdx.x == 0) stat0[out_r] = S0;
}

// ---- diff_pa_len_pairs / diff_pa_len_markers: every pair, every marker, each as diff_pa_len ---------------------------
// The items, their bits and the one compaction over all n positions are those of diff_pa_pairs and diff_pa_markers
// above; the test is k_rep_perm_len's on the item's OWN rows: the rows of the record with t_i > 0 in the item, in order,
// with w_i = x_i - min x and tol = 2^-40 (max x - min x) over those rows, x the rows' positions as passed.  A row
// without a read in the item is passed over, not multiplied by 0: its x may lie outside [min x, max x] of the item, its
// w outside [0, span].  Every sum goes through rep_len_row and rep_len_delta, so n_ge and the bits of delta(0) are those
// of k_rep_perm_len on the item's two populations.  The rounding comment above k_rep_perm_len (at most
// REP_LEN_MAX_ROWS rows, (4 R + 7) u span <= tol / 2) covers both kernels: an item's rows are a subset of the record's,
// at most 1,024 of them (checked by the entry points), and span is the item's own.
//
// How an item gets t_i, a_i(0) and a_i(p) of kept row i.  A pair: the two groups' columns of a0 [row][group], and the
// nonzeros of the two segments moved to the pair's local positions (the shifts of k_rep_perm_pairs)
struct RepLenPairRows {
    const int64_t *__restrict__ a0, *__restrict__ sg;
    const uint2 *__restrict__ nz;
    int n_groups, g, h, sh_g, sh_h;
    __device__ __forceinline__ int obs(int64_t i) const { return (int)a0[i * n_groups + g]; }
    __device__ __forceinline__ int reads(int64_t i) const { return obs(i) + (int)a0[i * n_groups + h]; }
    __device__ __forceinline__ int perm(int64_t i, const unsigned long long *__restrict__ mb, int64_t pstride) const {
        const int64_t *si = sg + i * (n_groups + 1);
        return rep_perm_segsum(nz, si[g], si[g + 1], sh_g, mb, pstride) +
               rep_perm_segsum(nz, si[h], si[h + 1], sh_h, mb, pstride);
    }
};
// a marker: t of the row over all tested cells, column g of a0 [row][segment], the whole row's nonzeros in slot order
struct RepLenMarkerRows {
    const int64_t *__restrict__ t, *__restrict__ a0, *__restrict__ noff;
    const uint2 *__restrict__ nz;
    int n_seg, g;
    __device__ __forceinline__ int obs(int64_t i) const { return (int)a0[i * n_seg + g]; }
    __device__ __forceinline__ int reads(int64_t i) const { return (int)t[i]; }
    __device__ __forceinline__ int perm(int64_t i, const unsigned long long *__restrict__ mb, int64_t pstride) const {
        return rep_perm_segsum(nz, noff[i], noff[i + 1], 0, mb, pstride);
    }
};

// The body of both kernels.  Workgroup = (item blockIdx.y of the range, record blockIdx.x / n_tiles, tile of 256
// permutations), one lane per permutation, registers only as k_rep_perm_len: no LDS, any number of rows in one launch.
// bits = the first mask word of the item.  Pass 1 reads the record's observed sums only (wave-uniform): T, A(0), the
// rows with t_i > 0 and min x, max x over them; the item does not test the record when fewer than two such rows remain,
// one of its populations has no read or span = 0, and then the workgroup stores delta(0) = 0.0 and leaves (uniform;
// no counter is touched).  Pass 2 walks each row with t_i > 0 once.  Exceedances by ballot, one atomic per wave into
// n_ge[item in range][record]; delta0 likewise, from tile 0.
template <typename Rows>
__device__ __forceinline__ void rep_perm_len_item(const Rows &rows, const unsigned long long *__restrict__ bits,
                                                  int32_t p_count, int32_t n_tiles, const int64_t *__restrict__ roff,
                                                  const double *__restrict__ x, int32_t n_rec,
                                                  int32_t *__restrict__ n_ge, double *__restrict__ delta0) {
#pragma clang fp contract(off)
    const int r = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles;
    const int64_t out_r = (int64_t)blockIdx.y * n_rec + r;
    const int64_t row0 = roff[r], row1 = roff[r + 1];
    long long T = 0, A0 = 0;
    int with_reads = 0;
    double xmin = 0.0, xmax = 0.0;
    for (int64_t i = row0; i < row1; ++i) {
        const int ti = rows.reads(i);
        if (ti == 0) continue;
        const double xi = x[i];
        xmin = with_reads && xmin <= xi ? xmin : xi;
        xmax = with_reads && xmax >= xi ? xmax : xi;
        T += ti;
        A0 += rows.obs(i);
        ++with_reads;
    }
    if (with_reads < 2 || A0 == 0 || A0 == T || !(xmax > xmin)) {
        if (tile == 0 && threadIdx.x == 0) delta0[out_r] = 0.0;
        return;
    }
    const double tol = (xmax - xmin) * 0x1p-40;
    const int p = tile * REP_THREADS + threadIdx.x;
    const bool valid = p < p_count;
    const unsigned long long *mb = bits + (valid ? p : p_count - 1);
    double W1 = 0.0, W2 = 0.0, V1 = 0.0, V2 = 0.0;
    long long A = 0, B = 0, B0 = 0;
    A0 = 0;
    for (int64_t i = row0; i < row1; ++i) {
        const int ti = rows.reads(i);
        if (ti == 0) continue;
        const double wi = x[i] - xmin;
        rep_len_row(rows.perm(i, mb, p_count), ti, wi, &W1, &W2, &A, &B);
        rep_len_row(rows.obs(i), ti, wi, &V1, &V2, &A0, &B0);
    }
    const double d = rep_len_delta(W1, W2, A, B), d0 = rep_len_delta(V1, V2, A0, B0);
    const unsigned long long b = __ballot(valid && fabs(d) >= fabs(d0) - tol);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&n_ge[out_r], __popcll(b));
    if (tile == 0 && threadIdx.x == 0) delta0[out_r] = d0;
}

// pairs = the descriptors from pair_first on; sg[i] = the row's G + 1 segment starts (k_rep_pair_segidx)
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_len_pairs(
    const unsigned long long *__restrict__ bits, int32_t p_count, int32_t n_tiles, const int64_t *__restrict__ roff,
    const int64_t *__restrict__ sg, const uint2 *__restrict__ nz, const int64_t *__restrict__ a0, int32_t n_groups,
    const int32_t *__restrict__ seg_off, const RepPair *__restrict__ pairs, const double *__restrict__ x, int32_t n_rec,
    int32_t *__restrict__ n_ge, double *__restrict__ delta0) {
    const RepPair pr = pairs[blockIdx.y];
    const RepLenPairRows rows{a0, sg, nz, n_groups, pr.g, pr.h, -seg_off[pr.g], pr.n_g - seg_off[pr.h]};
    rep_perm_len_item(rows, bits + (int64_t)pr.woff * p_count, p_count, n_tiles, roff, x, n_rec, n_ge, delta0);
}

// marker marker_first + blockIdx.y; n_words = the mask words of a marker and permutation
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_len_markers(
    const unsigned long long *__restrict__ bits, int32_t p_count, int32_t n_tiles, int32_t n_words,
    const int64_t *__restrict__ roff, const int64_t *__restrict__ noff, const uint2 *__restrict__ nz,
    const int64_t *__restrict__ t, const int64_t *__restrict__ a0, int32_t n_seg, int32_t marker_first,
    const double *__restrict__ x, int32_t n_rec, int32_t *__restrict__ n_ge, double *__restrict__ delta0) {
    const int g = marker_first + blockIdx.y;
    const RepLenMarkerRows rows{t, a0, noff, nz, n_seg, g};
    rep_perm_len_item(rows, bits + (int64_t)g * n_words * p_count, p_count, n_tiles, roff, x, n_rec, n_ge, delta0);
}

// ---- diff_pa_trend: pA usage along a per-cell score ---------------------------------------------------------------------
// The contract extends the G-way one.  The tested columns are the first n columns of the count matrix, position j =
// column j, 2 <= n < 2^24; q[0 .. n) are the observed integer scores of the positions, 0 <= q <= 32,768.  Permutation
// p >= 1 ranks the positions by the unchanged key(p, j): rho_p(j) = #{i : key(p, i) < key(p, j)} is a bijection, because
// keys are distinct, and position j receives the score z_p(j) = q[rho_p(j)].  When q[j] is the observed group index
// (non-decreasing in j), z_p(j) is byte for byte the label that k_rep_perm_labels writes.
#define REP_SCORE_MAX 32768
#define REP_SCORE_MIN_BUCKETS 1024     // a wave scans its quarter of the buckets in tiles of 64 x 4
#define REP_SCORE_MAX_BUCKETS 16384    // 64 KiB of LDS counters
#define REP_TREND_MAX_ROWS 4000

// one workgroup per permutation p_first + blockIdx.x: the rank of EVERY key, by buckets of the keys' top `bits` bits (B =
// 2^bits counters in LDS, chosen by the host: the smallest power of two that reaches n, within REP_SCORE_MIN_BUCKETS ..
// REP_SCORE_MAX_BUCKETS; the top 40 bits of a key are hash bits, so a bucket expects n / B positions).  Four passes over
// the n positions, the keys recomputed in every pass as rep_select_key does:
//   1  cnt[bucket of key(j)] += 1 (LDS atomics whose results are not used);
//   2  the exclusive scan of cnt in place: wave w adds up its quarter of the buckets, and behind a barrier scans it in
//      tiles of 256 buckets (an int4 per lane, the carry in a register) from the sum of the quarters before it;
//   3  slot = cnt[bucket]++ (a returning LDS atomic), members[slot] = j: every bucket's positions lie in its own slice
//      [start, end) of the permutation's n-int32 scratch slice, and behind the pass cnt[b] = end of bucket b = start of
//      bucket b + 1, so one array serves;
//   4  behind a barrier, rank(j) = start + #{members m of the bucket of j : key(m) < key(j)}, and the halfword
//      scores[j * p_count + blockIdx.x] = q[rank(j)]: the layout of the label bytes, lanes that own neighbouring
//      permutations read neighbouring halfwords.
// The order in which pass 3's atomics arrive decides where in its slice a member lies and nothing else: pass 4 reads the
// whole slice and COUNTS, and a count does not depend on the order of what is counted, so the ranks and the scores are
// the same in every run.  The barriers: cnt is zeroed, counted, scanned and filled behind one barrier each; the barrier
// between passes 3 and 4 also orders the workgroup's own global writes to `members` before its reads (a workgroup-scope
// release and acquire, which is what __syncthreads is), and no other workgroup touches the slice.  Every slot is below n
// (the counts add up to n) and so is every rank.
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_scores(int32_t n, int32_t bits, const uint16_t *__restrict__ q,
                                                                 unsigned long long p_first, int32_t p_count,
                                                                 unsigned long long seed, int32_t *members_all,
                                                                 uint16_t *__restrict__ scores) {
    extern __shared__ int32_t rep_cnt[];     // the B counters, then the waves' sums of the scan
    const unsigned long long base = rep_mix(seed + REP_PERM_G * (p_first + blockIdx.x));
    int32_t *members = members_all + (int64_t)blockIdx.x * n;
    const int n_buckets = 1 << bits, shift = 64 - bits;
    int32_t *wtot = rep_cnt + n_buckets;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int4 *cnt4 = reinterpret_cast<int4 *>(rep_cnt);
    for (int i = threadIdx.x; i < n_buckets / 4; i += REP_THREADS) cnt4[i] = make_int4(0, 0, 0, 0);
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += REP_THREADS) atomicAdd(&rep_cnt[rep_perm_key(base, j) >> shift], 1);
    __syncthreads();
    const int quarter4 = n_buckets / (4 * REP_WAVES);      // int4s per wave: a multiple of 64
    int4 *mine = cnt4 + wave * quarter4;
    int sum = 0;
    for (int i = lane; i < quarter4; i += 64) {
        const int4 h = mine[i];
        sum += h.x + h.y + h.z + h.w;
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) wtot[wave] = sum;
    __syncthreads();
    int run = 0;
    for (int w = 0; w < wave; ++w) run += wtot[w];
    for (int i = lane; i < quarter4; i += 64) {
        const int4 h = mine[i];
        const int tile = h.x + h.y + h.z + h.w;
        int incl = tile;
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        const int ex = run + incl - tile;
        mine[i] = make_int4(ex, ex + h.x, ex + h.x + h.y, ex + h.x + h.y + h.z);
        run += __shfl(incl, 63, 64);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += REP_THREADS) members[atomicAdd(&rep_cnt[rep_perm_key(base, j) >> shift], 1)] = j;
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += REP_THREADS) {
        const unsigned long long k = rep_perm_key(base, j);
        const int b = (int)(k >> shift);
        const int start = b ? rep_cnt[b - 1] : 0, end = rep_cnt[b];
        int rank = start;
        for (int m = start; m < end; ++m) rank += rep_perm_key(base, members[m]) < k;
        scores[(int64_t)j * p_count + blockIdx.x] = q[rank];
    }
}

// one permutation's column of the scores, gathered for scape_hip_report_perm_scores_get: a strided copy of n halfwords
// to the host takes a transfer per halfword
__global__ __launch_bounds__(REP_THREADS) void k_rep_scores_column(const uint16_t *__restrict__ scores, int32_t n,
                                                                   int32_t p_count, int32_t p, uint16_t *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * REP_THREADS + threadIdx.x;
    if (j < n) out[j] = scores[j * p_count + p];
}

// The statistic, per record with R kept rows, c_ij the count of row i at position j, under scores z:
//   t_i = sum_j c_ij (fixed),  T = sum_i t_i < 2^31,  s_i = sum_j c_ij z(j) (64-bit, exact, < 2^46),  S = sum_i s_i
//   D   = sum_i t_i (s_i / t_i - S / T)^2     (rows in order)  the between-site sum of squares of the score
//   d_i = s_i / t_i - (S - s_i) / (T - t_i)                    the mean score of site i's reads against the other reads'
// This is diff_pa_len_groups's arithmetic with the roles exchanged - site for group, score for position - and both the
// observed and the permuted scores go through rep_len_groups_term and rep_len_groups_delta (contraction off, equal
// integers give equal doubles), with m = (double)S / (double)T formed per labelling, since S now depends on it.  Their
// rounding analysis carries over with G -> R and qspan = max q <= 2^15: every integer converted is below 2^53,
//   |D - exact| <= (R + 8) u T qspan^2,     |d_i - exact| <= 3 u qspan     (u = 2^-53).
// A permutation is counted when D(p) >= D(0) - tolD, tolD = 2^-40 T qspan^2, and when |d_i(p)| >= |d_i(0)| - told, told =
// 2^-40 qspan.  A labelling whose exact statistic reaches the observed one is counted whatever the rounding, and one more
// than twice the band below it never is, as long as 2 eD + u T qspan^2 <= tolD: (2 R + 17) u <= 2^-40 = 8,192 u.  Here R
// is not bounded by 64 as G is, so a record may own at most REP_TREND_MAX_ROWS = 4,000 kept rows (checked by the entry
// point): 8,017 u, 175 u to spare.  d_i needs 7 u.  tolD = (double)(T qspan^2) 2^-40 rounds the integer (below 2^61) by
// at most u of itself, 2^-53 of the band.

// one workgroup per record: the observed scores q.  Wave w takes rows w, w + REP_WAVES, ...: s0[i] = s_i(0) and sq0[i] =
// sum_j c_ij q_j^2 (below 2^61; the host's eta2 needs their sum).  Then qt[2 r], qt[2 r + 1] = S(0), T; tol[2 r], tol[2
// r + 1] = tolD, told; d0[i] = d_i(0) by thread i, i + 256, ...; stat0[r] = D(0), the rows' terms added in order by one
// thread, as a lane of k_rep_perm_trend adds them
__global__ __launch_bounds__(REP_THREADS) void k_rep_trend_obs(const int64_t *__restrict__ roff,
                                                               const int64_t *__restrict__ noff,
                                                               const uint2 *__restrict__ nz,
                                                               const int64_t *__restrict__ t,
                                                               const uint16_t *__restrict__ q, int32_t qspan,
                                                               long long *s0, long long *__restrict__ sq0,
                                                               long long *__restrict__ qt, double *__restrict__ tol,
                                                               double *__restrict__ d0, double *__restrict__ stat0) {
#pragma clang fp contract(off)
    __shared__ long long ST[2];
    const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row0 = roff[r], row1 = roff[r + 1];
    for (int64_t i = row0 + wave; i < row1; i += REP_WAVES) {
        long long s = 0, sq = 0;
        for (int64_t k = noff[i] + lane; k < noff[i + 1]; k += 64) {
            const uint2 e = nz[k];
            const long long v = (long long)e.y * q[e.x];
            s += v;
            sq += v * q[e.x];
        }
        for (int o = 32; o > 0; o >>= 1) {
            s += __shfl_xor(s, o, 64);
            sq += __shfl_xor(sq, o, 64);
        }
        if (lane == 0) {
            s0[i] = s;
            sq0[i] = sq;
        }
    }
    __syncthreads();                         // the record's s0 are stored (this workgroup wrote them)
    if (threadIdx.x == 0) {
        long long S = 0, T = 0;
        for (int64_t i = row0; i < row1; ++i) {
            S += s0[i];
            T += t[i];
        }
        ST[0] = S;
        ST[1] = T;
    }
    __syncthreads();
    const long long S = ST[0], T = ST[1];
    for (int64_t i = row0 + threadIdx.x; i < row1; i += REP_THREADS) d0[i] = rep_len_groups_delta(s0[i], t[i], S, T);
    if (threadIdx.x == 0) {
        const double m = (double)S / (double)T;
        double D = 0.0;
        for (int64_t i = row0; i < row1; ++i) D = D + rep_len_groups_term(s0[i], t[i], m);
        qt[2 * r] = S;
        qt[2 * r + 1] = T;
        tol[2 * r] = ldexp((double)(T * qspan * qspan), -40);
        tol[2 * r + 1] = ldexp((double)qspan, -40);
        stat0[r] = D;
    }
}

// workgroup = (record blockIdx.x / n_tiles, tile of 256 permutations), one lane per permutation; the nonzeros are
// wave-uniform, the lane reads its own permutation's halfword of the nonzero's position (neighbouring lanes,
// neighbouring halfwords).  A first walk over all the record's nonzeros forms S(p) in a 64-bit register; a second walk,
// row by row, forms s_i(p) in a register and adds the row's term: no LDS, so any number of rows in one launch and no
// classes of records.  Exceedances are counted per wave (ballot) and added with one atomic per wave and counter.
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_trend(
    const uint16_t *__restrict__ scores, int32_t p_count, int32_t n_tiles, const int64_t *__restrict__ roff,
    const int64_t *__restrict__ noff, const uint2 *__restrict__ nz, const int64_t *__restrict__ t,
    const long long *__restrict__ qt, const double *__restrict__ tol, const double *__restrict__ d0,
    const double *__restrict__ stat0, int32_t *__restrict__ site_ge, int32_t *__restrict__ gene_ge) {
#pragma clang fp contract(off)
    const int r = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles;
    const int p = tile * REP_THREADS + threadIdx.x;
    const bool valid = p < p_count;
    const uint16_t *sc = scores + (valid ? p : p_count - 1);
    const int64_t row0 = roff[r], row1 = roff[r + 1];
    const long long T = qt[2 * r + 1];
    const double tolD = tol[2 * r], told = tol[2 * r + 1];
    long long S = 0;
    rep_groups_walk(nz, noff[row0], noff[row1], sc, p_count, [&](int z, int c) { S += (long long)z * c; });
    const double m = (double)S / (double)T;
    double D = 0.0;
    for (int64_t i = row0; i < row1; ++i) {
        long long s = 0;
        rep_groups_walk(nz, noff[i], noff[i + 1], sc, p_count, [&](int z, int c) { s += (long long)z * c; });
        const long long ti = t[i];
        D = D + rep_len_groups_term(s, ti, m);
        const double d = rep_len_groups_delta(s, ti, S, T);
        const unsigned long long b = __ballot(valid && fabs(d) >= fabs(d0[i]) - told);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(&site_ge[i], __popcll(b));
    }
    const unsigned long long b = __ballot(valid && D >= stat0[r] - tolD);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&gene_ge[r], __popcll(b));
}

// ---- diff_pa_len_trend: 3'UTR length along a per-cell score -----------------------------------------------------------
// The scores, their permutations and the kept rows are diff_pa_trend's; kept row i also has an integer position x_i,
// 0 <= x_i <= 2^22 (the host quantises alpha_arr per record).  Per record, under scores z:
//   t_i = sum_j c_ij,  T = sum_i t_i < 2^31,  Sx = sum_i t_i x_i                       (fixed)
//   s_i = sum_j c_ij z(j) < 2^46,  Sz = sum_i s_i,  Sxz = sum_i x_i s_i                (per labelling)
//   C   = T Sxz - Sx Sz     = T^2 x the covariance of position and score over the record's reads
// T, Sx and sum_i t_i x_i^2 do not depend on the labelling, so |C| orders the labellings as the absolute slope of the
// score regressed on the position does, and a permutation is counted when |C(p)| >= |C(0)|, compared as integers: no
// f64, no band.  The ranges: the entry point checks T max x < 2^48 per record, so Sx < 2^48, and with z <= 2^15 Sz <=
// 2^15 T < 2^46 and Sxz <= 2^15 T max x < 2^63: all of them fit signed 64-bit registers.  C is two 64 x 64 -> 128-bit
// products, each below 2^94, and their difference, in __int128; no division anywhere.
#define REP_LEN_TREND_MAX_TX ((long long)1 << 48)    // T max x of a record stays below it (x_i <= REP_LEN_GROUPS_MAX_Q)
#define REP_LEN_TREND_REC 6             // per record: T, Sx, Sz(0), Sxz(0), the low and the high 64 bits of C(0)

__device__ __forceinline__ unsigned __int128 rep_len_trend_abs(long long T, long long Sx, long long Sz, long long Sxz,
                                                               __int128 *C_out) {
    const __int128 C = (__int128)T * Sxz - (__int128)Sx * Sz;
    if (C_out) *C_out = C;
    return C < 0 ? (unsigned __int128)(-C) : (unsigned __int128)C;
}

// one workgroup per record: the observed scores q.  Wave w takes rows w, w + REP_WAVES, ...: s0[i] = s_i(0) and sq0[i] =
// sum_j c_ij q_j^2 (below 2^61; the host's slope and r need their sum), as k_rep_trend_obs.  Then one thread adds the
// rows up in order: rec[6 r ..] = T, Sx, Sz(0), Sxz(0), C(0) low, C(0) high
__global__ __launch_bounds__(REP_THREADS) void k_rep_len_trend_obs(const int64_t *__restrict__ roff,
                                                                   const int64_t *__restrict__ noff,
                                                                   const uint2 *__restrict__ nz,
                                                                   const int64_t *__restrict__ t,
                                                                   const int32_t *__restrict__ x,
                                                                   const uint16_t *__restrict__ q, long long *s0,
                                                                   long long *__restrict__ sq0,
                                                                   long long *__restrict__ rec) {
    const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row0 = roff[r], row1 = roff[r + 1];
    for (int64_t i = row0 + wave; i < row1; i += REP_WAVES) {
        long long s = 0, sq = 0;
        for (int64_t k = noff[i] + lane; k < noff[i + 1]; k += 64) {
            const uint2 e = nz[k];
            const long long v = (long long)e.y * q[e.x];
            s += v;
            sq += v * q[e.x];
        }
        for (int o = 32; o > 0; o >>= 1) {
            s += __shfl_xor(s, o, 64);
            sq += __shfl_xor(sq, o, 64);
        }
        if (lane == 0) {
            s0[i] = s;
            sq0[i] = sq;
        }
    }
    __syncthreads();                         // the record's s0 are stored (this workgroup wrote them)
    if (threadIdx.x == 0) {
        long long T = 0, Sx = 0, Sz = 0, Sxz = 0;
        for (int64_t i = row0; i < row1; ++i) {
            T += t[i];
            Sx += t[i] * x[i];
            Sz += s0[i];
            Sxz += x[i] * s0[i];
        }
        __int128 C;
        rep_len_trend_abs(T, Sx, Sz, Sxz, &C);
        long long *o = rec + (int64_t)REP_LEN_TREND_REC * r;
        o[0] = T;
        o[1] = Sx;
        o[2] = Sz;
        o[3] = Sxz;
        o[4] = (long long)(unsigned long long)(unsigned __int128)C;
        o[5] = (long long)(C >> 64);
    }
}

// workgroup = (record blockIdx.x / n_tiles, tile of 256 permutations), one lane per permutation, as k_rep_perm_trend; one
// walk over the record's rows: s_i(p) in a 64-bit register, then Sz += s_i and Sxz += x_i s_i.  Behind the last row the
// lane forms C(p), and the exceedances |C(p)| >= |C(0)| are counted per wave (ballot) and added with one atomic per
// wave.  No LDS, no f64.
__global__ __launch_bounds__(REP_THREADS) void k_rep_perm_len_trend(
    const uint16_t *__restrict__ scores, int32_t p_count, int32_t n_tiles, const int64_t *__restrict__ roff,
    const int64_t *__restrict__ noff, const uint2 *__restrict__ nz, const int32_t *__restrict__ x,
    const long long *__restrict__ rec, int32_t *__restrict__ gene_ge) {
    const int r = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles;
    const int p = tile * REP_THREADS + threadIdx.x;
    const bool valid = p < p_count;
    const uint16_t *sc = scores + (valid ? p : p_count - 1);
    const int64_t row0 = roff[r], row1 = roff[r + 1];
    const long long *o = rec + (int64_t)REP_LEN_TREND_REC * r;
    const long long T = o[0], Sx = o[1];
    const unsigned __int128 C0 = rep_len_trend_abs(T, Sx, o[2], o[3], nullptr);
    long long Sz = 0, Sxz = 0;
    for (int64_t i = row0; i < row1; ++i) {
        long long s = 0;
        rep_groups_walk(nz, noff[i], noff[i + 1], sc, p_count, [&](int z, int c) { s += (long long)z * c; });
        Sz += s;
        Sxz += x[i] * s;
    }
    const unsigned long long b = __ballot(valid && rep_len_trend_abs(T, Sx, Sz, Sxz, nullptr) >= C0);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&gene_ge[r], __popcll(b));
}

// ---- host side ------------------------------------------------------------------------------------------------------
// Every entry point below keeps the drain rule (StreamDrain, scape_hip.hip): the host memory its queued copies read or
// write sits in the base of a test's frame (RepPermHost goes after RepPermCall's drain) or is declared ahead of a
// builder's drain.

static const int32_t REP_PERM_CAPS[] = {4, 8, 16, 32, 64};   // rows of a record held in LDS at once (1 KiB each)
static const int REP_PERM_N_CAPS = (int)(sizeof(REP_PERM_CAPS) / sizeof(REP_PERM_CAPS[0]));

// the records by LDS class, for k_rep_perm_test, k_rep_perm_pairs and k_rep_perm_markers: the smallest cap that holds all of a record's rows
// (the largest cap takes the rest, in groups).  recs = the records in class order, count[q] = those of class q
struct RepPermClasses {
    std::vector<int32_t> recs;
    int64_t count[REP_PERM_N_CAPS];
};

static RepPermClasses rep_perm_classes(int32_t n_rec, const int64_t *rec_row_off) {
    std::vector<std::vector<int32_t>> by_cap(REP_PERM_N_CAPS);
    for (int r = 0; r < n_rec; ++r) {
        const int64_t k = rec_row_off[r + 1] - rec_row_off[r];
        int q = 0;
        while (q < REP_PERM_N_CAPS - 1 && k > REP_PERM_CAPS[q]) ++q;
        by_cap[q].push_back(r);
    }
    RepPermClasses cl;
    for (int q = 0; q < REP_PERM_N_CAPS; ++q) {
        cl.recs.insert(cl.recs.end(), by_cap[q].begin(), by_cap[q].end());
        cl.count[q] = (int64_t)by_cap[q].size();
    }
    return cl;
}

// what every builder of labellings asks of its n positions (`cells_must` names them: "... must [be]") and its chunk
static int rep_perm_chunk_ok(int64_t n, const char *cells_must, int64_t p_first, int32_t p_count) {
    if (n >= REP_PERM_MAX_N) return fail(std::string(cells_must) + " below 2^24 (a key keeps the position in 24 bits)");
    if (p_first < 1 || p_count < 1) return fail("p_first and p_count must be at least 1 (permutation 0 is the observed labelling)");
    return 0;
}

// A builder call refused by a check keeps the earlier labellings.  Behind its checks a builder sets count = 0 and arms
// its drain: from the first allocation on they are gone until rep_built() has waited for the kernel and recorded the new
static int rep_built(StreamDrain &drain, RepLabellings &l, int64_t n, int32_t p_count) {
    HIPCHK(hipGetLastError());
    if (drain.wait()) return 1;
    l.n = (int32_t)n, l.count = p_count;
    return 0;
}

// the membership bits of permutations p_first .. p_first + p_count - 1 for strata of m1[k] + m2[k] >= 1 cells (the
// entry points have checked each stratum)
static int rep_build_masks(scape_hip_ctx *c, int32_t n_strata, const int32_t *m1, const int32_t *m2, int64_t p_first,
                           int32_t p_count, uint64_t seed) {
    int64_t n1 = 0, n2 = 0;
    for (int32_t k = 0; k < n_strata; ++k) {
        n1 += m1[k];
        n2 += m2[k];
    }
    if (n1 < 1 || n2 < 1) return fail("both populations need at least one cell");
    if (rep_perm_chunk_ok(n1 + n2, "n1 + n2 must be", p_first, p_count)) return 1;
    ReportState *s = report_state(c);
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
    s->masks.count = 0;
    StreamDrain drain(c->stream);
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
    s->m_n1 = (int32_t)n1;
    return rep_built(drain, s->masks, n, p_count);
}

// the groups of a test on column segments are those of the builder's last call, which remembered their sizes
static int rep_groups_match(const RepLabellings &l, int32_t n_groups, const int32_t *seg_off) {
    if (!seg_off) return fail("bad argument");
    if (n_groups != (int32_t)l.sizes.size()) return fail("n_groups differs from the last " + std::string(l.builder) + " call");
    if (seg_off[0] != 0) return fail("seg_off must start at 0 (position j is column j)");
    for (int32_t g = 0; g < n_groups; ++g)
        if (seg_off[g + 1] - seg_off[g] != l.sizes[g])
            return fail("group " + std::to_string(g) + ": seg_off differs from the sizes of the last " + l.builder + " call");
    return 0;
}

// what the builders of G-way labellings and of pair masks ask of the groups: their number, and (sizes is there) their cells
static int rep_n_groups_ok(int32_t n_groups) {
    if (n_groups < 2 || n_groups > REP_GROUPS_MAX)
        return fail("n_groups must lie in 2 .. " + std::to_string(REP_GROUPS_MAX));
    return 0;
}

static int rep_group_sizes_ok(int32_t n_groups, const int32_t *sizes) {
    for (int32_t g = 0; g < n_groups; ++g)
        if (sizes[g] < 1) return fail("group " + std::to_string(g) + ": every group needs at least one cell");
    return 0;
}

// a `_get` entry point starts here; item_refused = the message where the pair or marker it names is none, else nullptr
static int rep_get_ok(const RepLabellings &l, const void *out, const char *item_refused, int32_t p) {
    if (l.built()) return 1;
    if (!out) return fail("bad argument");
    if (item_refused) return fail(item_refused);
    return l.holds(p);
}

// The frame of a test call behind RepLabellings::ready; an entry point sets what it uses.  n = the tested positions and
// p_count = the permutations of the labellings `what`.  Two populations (seg_off = nullptr): a0 = the row's sum over the
// positions below n1, in p_a0.  n_groups populations in the column segments seg_off: a0 = the n_groups sums of the row,
// in q_a0.  outs_ok = the caller's own other pointers are there; max_rec_rows > 0: a record may own at most that many
// rows; w / tol / tol2, when given, must be finite and not negative; the positions q, when given, lie in 0 .. 2^22; the
// positions x, when given, are finite and so is max x - min x of every record.
struct RepPermHost {                   // the call's host memory that queued copies read or write
    RepPermClasses classes;            // rep_perm_launch_classes
    std::vector<int32_t> site, gene;   // rep_perm_count: the counters of this chunk
    std::vector<int64_t> own_a0, lrec; // what single tests fetch for themselves: the trend tests' a0, len_trend's records
    std::vector<double> tols;          // len_groups: (tolD, told) per record, uploaded
};
struct RepPermCall : RepPermHost {
    int32_t n, p_count, n_rec, n1 = 0, n_groups = 0;
    const char *what;
    const int64_t *rec_row_off, *rows;
    int64_t *t_out, *a0_out = nullptr;
    const int32_t *seg_off = nullptr, *q = nullptr;
    const double *w = nullptr, *tol = nullptr, *tol2 = nullptr, *x = nullptr;
    bool outs_ok = false;
    int64_t max_rec_rows = 0;
    int32_t reads_bits = 31;           // a record has fewer than 2^reads_bits reads in the tested cells (boot_len: 27)
    int64_t n_rows = 0, nnz = 0;      // results of rep_perm_prepare: the kept rows, their nonzeros and the tiles of
    int32_t n_tiles = 0;               // REP_THREADS permutations
    StreamDrain drain;                 // waits, where armed, before the base goes
    RepPermCall(scape_hip_ctx *c, const RepLabellings &l, int32_t n_rec_, const int64_t *rec_row_off_, const int64_t *rows_,
                int64_t *t_out_)
        : n(l.n), p_count(l.count), n_rec(n_rec_), what(l.what), rec_row_off(rec_row_off_), rows(rows_), t_out(t_out_),
          drain(c->stream, false) {}
};

// the part the tests share: the checks, all of them before anything is queued on the device, then the upload of rows and
// offsets and the compaction of the kept rows to their nonzeros (p_noff / p_nz), with t and a0 of every row on the host
static int rep_perm_prepare(scape_hip_ctx *c, RepPermCall &k) {
    ReportState *s = c->rep;
    const int32_t n_rec = k.n_rec;
    const int64_t *rec_row_off = k.rec_row_off;
    if (n_rec <= 0 || !rec_row_off || !k.rows || !k.t_out || !k.a0_out || !k.outs_ok) return fail("bad argument");
    if (k.n > s->n_cols)
        return fail("the count matrix has fewer columns than the " + std::string(k.what) + " have positions");
    if (rec_row_off[0] != 0) return fail("rec_row_off must start at 0");
    for (int r = 0; r < n_rec; ++r)
        if (rec_row_off[r + 1] < rec_row_off[r]) return fail("rec_row_off must be non-decreasing");
    const int64_t n_rows = rec_row_off[n_rec];
    if (n_rows <= 0 || n_rows > INT32_MAX) return fail("rec_row_off must end at the row count, between 1 and 2^31 - 1");
    if (k.max_rec_rows > 0)
        for (int r = 0; r < n_rec; ++r)
            if (rec_row_off[r + 1] - rec_row_off[r] > k.max_rec_rows)
                return fail("record " + std::to_string(r) + ": more than " + std::to_string(k.max_rec_rows) + " rows");
    for (int64_t i = 0; i < n_rows; ++i)
        if (k.rows[i] < 0 || k.rows[i] >= s->n_cnt_rows) return fail("row index out of range");
    const int32_t n_tiles = (k.p_count + REP_THREADS - 1) / REP_THREADS;
    if ((int64_t)n_rec * n_tiles > INT32_MAX) return fail("too many records x permutation tiles for one call");
    for (int64_t i = 0; k.w && i < n_rows; ++i)
        if (!(k.w[i] >= 0.0) || std::isinf(k.w[i])) return fail("row weights must be finite and not negative");
    for (const double *tl : {k.tol, k.tol2})
        for (int r = 0; tl && r < n_rec; ++r)
            if (!(tl[r] >= 0.0) || std::isinf(tl[r])) return fail("tolerances must be finite and not negative");
    for (int64_t i = 0; k.q && i < n_rows; ++i)
        if (k.q[i] < 0 || k.q[i] > REP_LEN_GROUPS_MAX_Q) return fail("row positions must lie in 0 .. 2^22");
    for (int r = 0; k.x && r < n_rec; ++r) {
        double lo = INFINITY, hi = -INFINITY;
        for (int64_t i = rec_row_off[r]; i < rec_row_off[r + 1]; ++i) {
            if (!std::isfinite(k.x[i])) return fail("record " + std::to_string(r) + ": row positions must be finite");
            lo = std::min(lo, k.x[i]), hi = std::max(hi, k.x[i]);
        }
        if (rec_row_off[r + 1] > rec_row_off[r] && !std::isfinite(hi - lo))
            return fail("record " + std::to_string(r) + ": the span of the row positions must be finite");
    }

    DevBuf &a0 = k.seg_off ? s->q_a0 : s->p_a0;
    const int64_t a0_bytes = n_rows * (k.seg_off ? k.n_groups : 1) * 8;
    if (s->p_rows.ensure(n_rows * 8) || s->p_roff.ensure(((int64_t)n_rec + 1) * 8) || s->p_nnz.ensure(n_rows * 8) ||
        s->p_noff.ensure((n_rows + 1) * 8) || s->p_t.ensure(n_rows * 8) || a0.ensure(a0_bytes) ||
        s->p_gene.ensure((int64_t)n_rec * 4) || s->p_stat0.ensure((int64_t)n_rec * 8))
        return 1;
    k.drain.armed = true;
    HIPCHK(hipMemcpyAsync(s->p_rows.p, k.rows, n_rows * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->p_roff.p, rec_row_off, ((int64_t)n_rec + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (k.seg_off) {
        if (s->q_seg.ensure(((int64_t)k.n_groups + 1) * 4)) return 1;
        HIPCHK(hipMemcpyAsync(s->q_seg.p, k.seg_off, ((int64_t)k.n_groups + 1) * 4, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_rep_groups_rowstat, dim3((uint32_t)n_rows), dim3(REP_THREADS), 0, c->stream,
                           s->p_rows.as<int64_t>(), s->n_cols, s->r_cnt.as<int32_t>(), k.n_groups, s->q_seg.as<int32_t>(),
                           s->p_nnz.as<int64_t>(), s->p_t.as<int64_t>(), a0.as<int64_t>());
    } else {
        hipLaunchKernelGGL(k_rep_perm_rowstat, dim3((uint32_t)n_rows), dim3(REP_THREADS), 0, c->stream,
                           s->p_rows.as<int64_t>(), s->n_cols, s->r_cnt.as<int32_t>(), k.n1, k.n, s->p_nnz.as<int64_t>(),
                           s->p_t.as<int64_t>(), a0.as<int64_t>());
    }
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rep_scan, dim3(1), dim3(REP_SCAN_THREADS), 0, c->stream, s->p_nnz.as<int64_t>(),
                       (int32_t)n_rows, s->p_noff.as<int64_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&k.nnz, s->p_noff.as<int64_t>() + n_rows, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(k.t_out, s->p_t.p, n_rows * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(k.a0_out, a0.p, a0_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int r = 0; r < n_rec; ++r) {
        int64_t T = 0;
        for (int64_t i = rec_row_off[r]; i < rec_row_off[r + 1]; ++i) T += k.t_out[i];
        if (T >= (int64_t)1 << k.reads_bits)
            return fail("record " + std::to_string(r) + ": 2^" + std::to_string(k.reads_bits) +
                        " or more reads in the tested cells");
    }
    if (s->p_nz.ensure(std::max<int64_t>(k.nnz, 1) * 8)) return 1;
    hipLaunchKernelGGL(k_rep_perm_fill, dim3((uint32_t)n_rows), dim3(REP_THREADS), 0, c->stream,
                       s->p_rows.as<int64_t>(), s->n_cols, s->r_cnt.as<int32_t>(), k.n, s->p_noff.as<int64_t>(),
                       s->p_nz.as<uint2>());
    HIPCHK(hipGetLastError());
    k.n_rows = n_rows, k.n_tiles = n_tiles;
    return 0;
}

// the tail of the tests: the exceedance counters p_site (n_site of them; none when 0) and p_gene (n_out) are zeroed,
// launch() queues the test, and the counts of this chunk of permutations are added to the caller's running totals;
// stat0_out, when given, gets p_stat0
template <typename Launch>
static int rep_perm_count(scape_hip_ctx *c, RepPermCall &k, int64_t n_site, int32_t n_out, int64_t *site_n_ge_out,
                          int64_t *gene_n_ge_out, double *stat0_out, Launch launch) {
    ReportState *s = c->rep;
    if (n_site && s->p_site.ensure(n_site * 4)) return 1;
    if (n_site) HIPCHK(hipMemsetAsync(s->p_site.p, 0, n_site * 4, c->stream));
    HIPCHK(hipMemsetAsync(s->p_gene.p, 0, (int64_t)n_out * 4, c->stream));
    if (launch()) return 1;
    k.site.resize(n_site), k.gene.resize(n_out);
    if (n_site) HIPCHK(hipMemcpyAsync(k.site.data(), s->p_site.p, n_site * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(k.gene.data(), s->p_gene.p, (int64_t)n_out * 4, hipMemcpyDeviceToHost, c->stream));
    if (stat0_out) HIPCHK(hipMemcpyAsync(stat0_out, s->p_stat0.p, (int64_t)n_out * 8, hipMemcpyDeviceToHost, c->stream));
    if (k.drain.wait()) return 1;
    for (int64_t i = 0; i < n_site; ++i) site_n_ge_out[i] += k.site[i];
    for (int r = 0; r < n_out; ++r) gene_n_ge_out[r] += k.gene[r];
    return 0;
}

// one launch of `kernel` per class of the call's records that has any: launch(records of the class on the device, their
// number, cap, bytes of dynamic LDS) queues it
template <typename Kernel, typename Launch>
static int rep_perm_launch_classes(scape_hip_ctx *c, RepPermCall &k, Kernel kernel, Launch launch) {
    ReportState *s = c->rep;
    const RepPermClasses &cl = k.classes = rep_perm_classes(k.n_rec, k.rec_row_off);
    HIPCHK(hipMemcpyAsync(s->p_recs.p, cl.recs.data(), (int64_t)cl.recs.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               REP_PERM_CAPS[REP_PERM_N_CAPS - 1] * REP_THREADS * 4));
    int64_t first = 0;
    for (int q = 0; q < REP_PERM_N_CAPS; ++q) {
        if (!cl.count[q]) continue;
        const int32_t cap = REP_PERM_CAPS[q];
        launch(s->p_recs.as<int32_t>() + first, cl.count[q], cap, (size_t)cap * REP_THREADS * 4);
        HIPCHK(hipGetLastError());
        first += cl.count[q];
    }
    return 0;
}

// what a test of a range of items (pairs, markers) checks first: ready, the groups' match and the range
// [first, first + count) of the builder's n_items
static int rep_ranged_ok(scape_hip_ctx *c, const RepLabellings &l, const std::string &noun, int32_t n_items,
                         int32_t first, int32_t count, int32_t n_rec, const int64_t *rec_row_off, int32_t n_groups,
                         const int32_t *seg_off) {
    if (l.ready(c->rep->n_cnt_rows) || rep_groups_match(l, n_groups, seg_off)) return 1;
    if (first < 0 || count < 1 || first > n_items - count)
        return fail(noun + "_first and " + noun + "_count must name " + noun + "s of the last " + l.builder + " call");
    if (n_rec > 0 && rec_row_off && ((int64_t)count * n_rec > INT32_MAX || rec_row_off[n_rec] > INT64_MAX / 8 / count))
        return fail("too many " + noun + "s x records or " + noun + "s x rows for one call: take the " + noun +
                    "s in ranges");
    return 0;
}

// The two tests of every item (pair, marker) of a range against the one compaction, by LDS class of records: behind
// rep_ranged_ok, prepare, the counters of count x n_rec; pre(k) checks, allocates and queues what the kernel needs
// first, launch(k, recs, m, cap, lds) one class
template <typename Kernel, typename Pre, typename Launch>
static int rep_perm_ranged(scape_hip_ctx *c, const RepLabellings &l, const std::string &noun, int32_t n_items,
                           int32_t first, int32_t count, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                           int32_t n_groups, const int32_t *seg_off, int64_t *t_out, int64_t *a0_out,
                           int64_t *site_n_ge_out, double *stat0_out, int64_t *gene_n_ge_out, Kernel kernel, Pre pre,
                           Launch launch) {
    ReportState *s = c->rep;
    if (rep_ranged_ok(c, l, noun, n_items, first, count, n_rec, rec_row_off, n_groups, seg_off)) return 1;
    RepPermCall k(c, l, n_rec, rec_row_off, rows, t_out);
    k.a0_out = a0_out, k.n_groups = n_groups, k.seg_off = seg_off, k.outs_ok = site_n_ge_out && stat0_out && gene_n_ge_out;
    if (rep_perm_prepare(c, k) || pre(k)) return 1;
    const int64_t n_out = (int64_t)count * n_rec;
    if (s->p_recs.ensure((int64_t)n_rec * 4) || s->p_gene.ensure(n_out * 4) || s->p_stat0.ensure(n_out * 8)) return 1;
    return rep_perm_count(c, k, count * k.n_rows, (int32_t)n_out, site_n_ge_out, gene_n_ge_out, stat0_out, [&]() -> int {
        return rep_perm_launch_classes(c, k, kernel, [&](const int32_t *recs, int64_t m, int32_t cap, size_t lds) {
            launch(k, recs, m, cap, lds);
        });
    });
}

// The test of the mean pA position by every item of a range, on the item's own rows: the checks of rep_perm_ranged and,
// in prepare, those of the positions x and of REP_LEN_MAX_ROWS, all before anything is queued; no LDS classes and no
// site counters; pre(k) as above, launch(k) queues the one kernel
template <typename Pre, typename Launch>
static int rep_perm_len_ranged(scape_hip_ctx *c, const RepLabellings &l, const std::string &noun, int32_t n_items,
                               int32_t first, int32_t count, int32_t n_rec, const int64_t *rec_row_off,
                               const int64_t *rows, int32_t n_groups, const int32_t *seg_off, const double *x,
                               int64_t *t_out, int64_t *a0_out, double *delta0_out, int64_t *n_ge_out, Pre pre,
                               Launch launch) {
    ReportState *s = c->rep;
    if (rep_ranged_ok(c, l, noun, n_items, first, count, n_rec, rec_row_off, n_groups, seg_off)) return 1;
    RepPermCall k(c, l, n_rec, rec_row_off, rows, t_out);
    k.a0_out = a0_out, k.n_groups = n_groups, k.seg_off = seg_off, k.x = x, k.max_rec_rows = REP_LEN_MAX_ROWS;
    k.outs_ok = x && delta0_out && n_ge_out;
    if (rep_perm_prepare(c, k) || pre(k)) return 1;
    const int64_t n_out = (int64_t)count * n_rec;
    if (s->l_w.ensure(k.n_rows * 8) || s->p_gene.ensure(n_out * 4) || s->p_stat0.ensure(n_out * 8)) return 1;
    return rep_perm_count(c, k, 0, (int32_t)n_out, nullptr, n_ge_out, delta0_out, [&]() -> int {
        HIPCHK(hipMemcpyAsync(s->l_w.p, x, k.n_rows * 8, hipMemcpyHostToDevice, c->stream));
        launch(k);
        HIPCHK(hipGetLastError());
        return 0;
    });
}

// per kept row and group the first nonzero of the group's segment, in x_seg, for the tests of pairs
static int rep_pair_segments(scape_hip_ctx *c, const RepPermCall &k, int32_t n_groups) {
    ReportState *s = c->rep;
    const int64_t n_seg = k.n_rows * (n_groups + 1);
    if ((n_seg + REP_THREADS - 1) / REP_THREADS > INT32_MAX) return fail("too many rows x groups for one call");
    if (s->x_seg.ensure(n_seg * 8)) return 1;
    hipLaunchKernelGGL(k_rep_pair_segidx, dim3((uint32_t)((n_seg + REP_THREADS - 1) / REP_THREADS)), dim3(REP_THREADS),
                       0, c->stream, s->p_noff.as<int64_t>(), s->p_nz.as<uint2>(), s->q_seg.as<int32_t>(), n_groups,
                       k.n_rows, s->x_seg.as<int64_t>());
    HIPCHK(hipGetLastError());
    return 0;
}

// the head of the two tests on scores: one segment [0, n), whose row sums restate t and land in the call's own buffer
static int rep_trend_prepare(scape_hip_ctx *c, RepPermCall &k) {
    if (k.n_rec <= 0 || !k.rec_row_off || !k.rows) return fail("bad argument");
    const int64_t n_all = k.rec_row_off[k.n_rec];
    if (n_all <= 0 || n_all > INT32_MAX) return fail("rec_row_off must end at the row count, between 1 and 2^31 - 1");
    k.own_a0.resize((size_t)n_all);
    k.a0_out = k.own_a0.data(), k.n1 = k.n;
    return rep_perm_prepare(c, k);
}

extern "C" {

int scape_hip_report_perm_masks(scape_hip_ctx *c, int32_t n1, int32_t n2, int64_t p_first, int32_t p_count,
                                uint64_t seed) {
    CTX_ENTER(c);
    return rep_build_masks(c, 1, &n1, &n2, p_first, p_count, seed);   // one stratum of every cell
}

int scape_hip_report_perm_masks_strata(scape_hip_ctx *c, int32_t n_strata, const int32_t *m1, const int32_t *m2,
                                       int64_t p_first, int32_t p_count, uint64_t seed) {
    CTX_ENTER(c);
    if (n_strata < 1 || !m1 || !m2) return fail("at least one stratum, with m1 and m2, is needed");
    for (int32_t s = 0; s < n_strata; ++s) {
        if (m1[s] < 0 || m2[s] < 0) return fail("stratum " + std::to_string(s) + ": a negative number of cells");
        if ((int64_t)m1[s] + m2[s] < 1) return fail("stratum " + std::to_string(s) + ": no cell");
    }
    return rep_build_masks(c, n_strata, m1, m2, p_first, p_count, seed);
}

int scape_hip_report_perm_bits_get(scape_hip_ctx *c, int32_t p, uint64_t *words_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    const RepLabellings &l = s->masks;
    if (rep_get_ok(l, words_out, nullptr, p)) return 1;
    StreamDrain drain(c->stream);
    HIPCHK(hipMemcpy2DAsync(words_out, 8, s->m_bits.as<unsigned long long>() + p, (size_t)l.count * 8, 8, (l.n + 63) / 64,
                            hipMemcpyDeviceToHost, c->stream));
    return drain.wait();
}

int scape_hip_report_perm_test(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                               int64_t *t_out, int64_t *a0_out, int64_t *site_n_ge_out, double *stat0_out,
                               int64_t *gene_n_ge_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    if (s->masks.ready(s->n_cnt_rows)) return 1;
    RepPermCall k(c, s->masks, n_rec, rec_row_off, rows, t_out);
    k.a0_out = a0_out, k.n1 = s->m_n1, k.outs_ok = site_n_ge_out && stat0_out && gene_n_ge_out;
    if (rep_perm_prepare(c, k) || s->p_recs.ensure((int64_t)n_rec * 4)) return 1;
    return rep_perm_count(c, k, k.n_rows, n_rec, site_n_ge_out, gene_n_ge_out, stat0_out, [&]() -> int {
        return rep_perm_launch_classes(c, k, k_rep_perm_test, [&](const int32_t *recs, int64_t m, int32_t cap,
                                                                   size_t lds) {
            hipLaunchKernelGGL(k_rep_perm_test, dim3((uint32_t)(m * k.n_tiles)), dim3(REP_THREADS), lds, c->stream,
                               s->m_bits.as<unsigned long long>(), k.p_count, k.n_tiles, recs, s->p_roff.as<int64_t>(),
                               s->p_noff.as<int64_t>(), s->p_nz.as<uint2>(), s->p_t.as<int64_t>(), s->p_a0.as<int64_t>(),
                               cap, s->p_site.as<int32_t>(), s->p_gene.as<int32_t>(), s->p_stat0.as<double>());
        });
    });
}

int scape_hip_report_perm_len(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                              const double *w, const double *tol, int64_t *t_out, int64_t *a0_out, double *delta0_out,
                              int64_t *n_ge_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    if (s->masks.ready(s->n_cnt_rows)) return 1;
    RepPermCall k(c, s->masks, n_rec, rec_row_off, rows, t_out);
    k.a0_out = a0_out, k.n1 = s->m_n1, k.max_rec_rows = REP_LEN_MAX_ROWS, k.w = w, k.tol = tol;
    k.outs_ok = w && tol && delta0_out && n_ge_out;
    if (rep_perm_prepare(c, k) || s->l_w.ensure(k.n_rows * 8) || s->l_tol.ensure((int64_t)n_rec * 8)) return 1;
    return rep_perm_count(c, k, 0, n_rec, nullptr, n_ge_out, delta0_out, [&]() -> int {
        HIPCHK(hipMemcpyAsync(s->l_w.p, w, k.n_rows * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(s->l_tol.p, tol, (int64_t)n_rec * 8, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_rep_perm_len, dim3((uint32_t)((int64_t)n_rec * k.n_tiles)), dim3(REP_THREADS), 0, c->stream,
                           s->m_bits.as<unsigned long long>(), k.p_count, k.n_tiles, s->p_roff.as<int64_t>(),
                           s->p_noff.as<int64_t>(), s->p_nz.as<uint2>(), s->p_t.as<int64_t>(), s->p_a0.as<int64_t>(),
                           s->l_w.as<double>(), s->l_tol.as<double>(), s->p_gene.as<int32_t>(),
                           s->p_stat0.as<double>());
        HIPCHK(hipGetLastError());
        return 0;
    });
}

int scape_hip_report_perm_labels(scape_hip_ctx *c, int32_t n_groups, const int32_t *sizes, int64_t p_first,
                                 int32_t p_count, uint64_t seed) {
    CTX_ENTER(c);
    if (rep_n_groups_ok(n_groups)) return 1;
    if (!sizes) return fail("bad argument");
    if (rep_group_sizes_ok(n_groups, sizes)) return 1;
    int64_t n = 0;
    for (int32_t g = 0; g < n_groups; ++g) n += sizes[g];
    if (rep_perm_chunk_ok(n, "the groups' cells must number", p_first, p_count)) return 1;
    ReportState *s = report_state(c);
    std::vector<int32_t> rank_of_cut(n_groups - 1);
    int32_t below = 0;
    for (int32_t h = 0; h + 1 < n_groups; ++h) {
        below += sizes[h];
        rank_of_cut[h] = below - 1;
    }
    s->labels.count = 0;
    StreamDrain drain(c->stream);
    if (s->q_lab.ensure((int64_t)p_count * n) || s->q_cut.ensure((int64_t)(n_groups - 1) * 4)) return 1;
    HIPCHK(hipMemcpyAsync(s->q_cut.p, rank_of_cut.data(), (int64_t)(n_groups - 1) * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_rep_perm_labels, dim3(p_count), dim3(REP_THREADS), 0, c->stream, n_groups,
                       s->q_cut.as<int32_t>(), (int32_t)n, (unsigned long long)p_first, p_count,
                       (unsigned long long)seed, s->q_lab.as<uint8_t>());
    s->labels.sizes.assign(sizes, sizes + n_groups);
    return rep_built(drain, s->labels, n, p_count);
}

int scape_hip_report_perm_labels_get(scape_hip_ctx *c, int32_t p, uint8_t *labels_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    const RepLabellings &l = s->labels;
    if (rep_get_ok(l, labels_out, nullptr, p)) return 1;
    StreamDrain drain(c->stream);
    HIPCHK(hipMemcpy2DAsync(labels_out, 1, s->q_lab.as<uint8_t>() + p, (size_t)l.count, 1, (size_t)l.n,
                            hipMemcpyDeviceToHost, c->stream));
    return drain.wait();
}

int scape_hip_report_perm_groups(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                 int32_t n_groups, const int32_t *seg_off, int64_t *t_out, int64_t *a0_out,
                                 int64_t *site_n_ge_out, double *stat0_out, double *site_stat0_out,
                                 int64_t *gene_n_ge_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    if (s->labels.ready(s->n_cnt_rows)) return 1;
    if (n_rec <= 0 || !rec_row_off) return fail("bad argument");   // what the check of the rounding bound reads
    if (rep_groups_match(s->labels, n_groups, seg_off)) return 1;
    for (int r = 0; r < n_rec; ++r)
        if (rec_row_off[r + 1] - rec_row_off[r] + n_groups > REP_GROUPS_MAX_ROWS_AND_GROUPS)
            return fail("record " + std::to_string(r) + ": " + std::to_string(rec_row_off[r + 1] - rec_row_off[r]) +
                        " rows and " + std::to_string(n_groups) + " groups, together more than " +
                        std::to_string(REP_GROUPS_MAX_ROWS_AND_GROUPS) + " (the rounding bound of the statistic)");
    RepPermCall k(c, s->labels, n_rec, rec_row_off, rows, t_out);
    k.a0_out = a0_out, k.n_groups = n_groups, k.seg_off = seg_off;
    k.outs_ok = site_n_ge_out && stat0_out && site_stat0_out && gene_n_ge_out;
    if (rep_perm_prepare(c, k)) return 1;
    const int64_t n_rows = k.n_rows;
    if (s->q_s0.ensure(n_rows * 8) || s->q_share.ensure(n_rows * 8)) return 1;
    return rep_perm_count(c, k, n_rows, n_rec, site_n_ge_out, gene_n_ge_out, stat0_out, [&]() -> int {
        hipLaunchKernelGGL(k_rep_groups_obs, dim3((uint32_t)n_rec), dim3(REP_THREADS), 0, c->stream,
                           s->p_roff.as<int64_t>(), s->p_t.as<int64_t>(), s->q_a0.as<int64_t>(), n_groups,
                           s->q_s0.as<double>(), s->q_share.as<double>(), s->p_stat0.as<double>());
        HIPCHK(hipGetLastError());
        const size_t lds = (size_t)2 * n_groups * REP_THREADS * 4;   // above 64 KiB a kernel needs the attribute
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_rep_perm_groups),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 2 * REP_GROUPS_MAX * REP_THREADS * 4));
        hipLaunchKernelGGL(k_rep_perm_groups, dim3((uint32_t)((int64_t)n_rec * k.n_tiles)), dim3(REP_THREADS), lds,
                           c->stream, s->q_lab.as<uint8_t>(), k.p_count, k.n_tiles, n_groups, s->p_roff.as<int64_t>(),
                           s->p_noff.as<int64_t>(), s->p_nz.as<uint2>(), s->p_t.as<int64_t>(), s->q_s0.as<double>(),
                           s->p_stat0.as<double>(), s->p_site.as<int32_t>(), s->p_gene.as<int32_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(site_stat0_out, s->q_share.p, n_rows * 8, hipMemcpyDeviceToHost, c->stream));
        return 0;
    });
}

int scape_hip_report_perm_len_groups(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                     int32_t n_groups, const int32_t *seg_off, const int32_t *q, const double *tol_stat,
                                     const double *tol_delta, int64_t *t_out, int64_t *a0_out, double *stat0_out,
                                     double *delta0_out, int64_t *n_ge_out, int64_t *group_n_ge_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    if (s->labels.ready(s->n_cnt_rows) || rep_groups_match(s->labels, n_groups, seg_off)) return 1;
    RepPermCall k(c, s->labels, n_rec, rec_row_off, rows, t_out);
    k.a0_out = a0_out, k.n_groups = n_groups, k.seg_off = seg_off, k.tol = tol_stat, k.tol2 = tol_delta, k.q = q;
    k.outs_ok = q && tol_stat && tol_delta && stat0_out && delta0_out && n_ge_out && group_n_ge_out;
    if (rep_perm_prepare(c, k)) return 1;
    const int64_t n_rows = k.n_rows, n_pairs = (int64_t)n_rec * n_groups;
    if (s->v_q.ensure(n_rows * 4) || s->v_tol.ensure((int64_t)n_rec * 16) || s->v_qt.ensure((int64_t)n_rec * 16) ||
        s->v_mean.ensure((int64_t)n_rec * 8) || s->v_d0.ensure(n_pairs * 8))
        return 1;
    for (int r = 0; r < n_rec; ++r) k.tols.insert(k.tols.end(), {tol_stat[r], tol_delta[r]});
    // equal slices of at most REP_LEN_GROUPS_SLICE groups: 33 groups take 17 + 16, not 32 + 1
    const int32_t n_slices = (n_groups + REP_LEN_GROUPS_SLICE - 1) / REP_LEN_GROUPS_SLICE;
    const int32_t slice = (n_groups + n_slices - 1) / n_slices;
    return rep_perm_count(c, k, n_pairs, n_rec, group_n_ge_out, n_ge_out, stat0_out, [&]() -> int {
        HIPCHK(hipMemcpyAsync(s->v_q.p, q, n_rows * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(s->v_tol.p, k.tols.data(), (int64_t)n_rec * 16, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_rep_len_groups_obs, dim3((uint32_t)n_rec), dim3(REP_THREADS), 0, c->stream,
                           s->p_roff.as<int64_t>(), s->p_t.as<int64_t>(), s->q_a0.as<int64_t>(), n_groups,
                           s->v_q.as<int32_t>(), s->v_qt.as<long long>(), s->v_mean.as<double>(), s->v_d0.as<double>(),
                           s->p_stat0.as<double>());
        HIPCHK(hipGetLastError());
        const size_t lds = (size_t)slice * REP_THREADS * 12;         // above 64 KiB a kernel needs the attribute
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_rep_perm_len_groups),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   REP_LEN_GROUPS_SLICE * REP_THREADS * 12));
        hipLaunchKernelGGL(k_rep_perm_len_groups, dim3((uint32_t)((int64_t)n_rec * k.n_tiles)), dim3(REP_THREADS), lds,
                           c->stream, s->q_lab.as<uint8_t>(), k.p_count, k.n_tiles, n_groups, slice,
                           s->p_roff.as<int64_t>(), s->p_noff.as<int64_t>(), s->p_nz.as<uint2>(), s->v_q.as<int32_t>(),
                           s->v_qt.as<long long>(), s->v_mean.as<double>(), s->v_d0.as<double>(),
                           s->p_stat0.as<double>(), s->v_tol.as<double>(), s->p_site.as<int32_t>(),
                           s->p_gene.as<int32_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(delta0_out, s->v_d0.p, n_pairs * 8, hipMemcpyDeviceToHost, c->stream));
        return 0;
    });
}

int scape_hip_report_perm_pair_masks(scape_hip_ctx *c, int32_t n_groups, const int32_t *sizes, int32_t n_pairs,
                                     const int32_t *pair_g, const int32_t *pair_h, int64_t p_first, int32_t p_count,
                                     uint64_t seed) {
    CTX_ENTER(c);
    if (rep_n_groups_ok(n_groups)) return 1;
    if (n_pairs < 1 || n_pairs > REP_GROUPS_MAX * (REP_GROUPS_MAX - 1) / 2)
        return fail("n_pairs must lie in 1 .. " + std::to_string(REP_GROUPS_MAX * (REP_GROUPS_MAX - 1) / 2));
    if (!sizes || !pair_g || !pair_h) return fail("bad argument");
    if (rep_group_sizes_ok(n_groups, sizes)) return 1;
    std::vector<int32_t> pairs((size_t)n_pairs * 8, 0);
    int64_t words = 0;
    for (int32_t k = 0; k < n_pairs; ++k) {
        const int32_t g = pair_g[k], h = pair_h[k];
        if (g < 0 || h >= n_groups || g >= h)
            return fail("pair " + std::to_string(k) + ": the groups must satisfy 0 <= g < h < n_groups");
        const int64_t n = (int64_t)sizes[g] + sizes[h];
        if (rep_perm_chunk_ok(n, "a pair's cells must number", p_first, p_count)) return 1;
        int32_t *d = &pairs[(size_t)k * 8];
        d[0] = g, d[1] = h, d[2] = sizes[g], d[3] = sizes[h], d[4] = (int32_t)words;
        words += (n + 63) / 64;
        if (words > INT32_MAX) return fail("the pairs' mask words together must number below 2^31");
    }
    ReportState *s = report_state(c);
    s->pair_masks.count = 0;
    StreamDrain drain(c->stream);
    if (s->x_bits.ensure(words * p_count * 8) || s->x_bound.ensure((int64_t)n_pairs * p_count * 8) ||
        s->x_desc.ensure((int64_t)n_pairs * 32))
        return 1;
    HIPCHK(hipMemcpyAsync(s->x_desc.p, pairs.data(), (int64_t)n_pairs * 32, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_rep_perm_pair_masks, dim3(p_count, n_pairs), dim3(REP_THREADS), 0, c->stream,
                       s->x_desc.as<RepPair>(), (unsigned long long)p_first, p_count, (unsigned long long)seed,
                       s->x_bound.as<unsigned long long>(), s->x_bits.as<unsigned long long>());
    s->pair_masks.sizes.assign(sizes, sizes + n_groups);
    int64_t n_all = 0;                       // the positions of a test on these masks: every group's cells
    for (int32_t g = 0; g < n_groups; ++g) n_all += sizes[g];
    s->x_pairs.swap(pairs);                  // the upload reads them where they now live
    return rep_built(drain, s->pair_masks, n_all, p_count);
}

int scape_hip_report_perm_pair_bits_get(scape_hip_ctx *c, int32_t pair, int32_t p, uint64_t *words_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    const RepLabellings &l = s->pair_masks;
    const bool pair_ok = pair >= 0 && pair < (int32_t)(s->x_pairs.size() / 8);
    if (rep_get_ok(l, words_out, pair_ok ? nullptr : "pair must name a pair of the last pair masks call", p)) return 1;
    const int32_t *d = &s->x_pairs[(size_t)pair * 8];
    const int32_t n_words = (d[2] + d[3] + 63) / 64;
    StreamDrain drain(c->stream);
    HIPCHK(hipMemcpy2DAsync(words_out, 8, s->x_bits.as<unsigned long long>() + (int64_t)d[4] * l.count + p,
                            (size_t)l.count * 8, 8, n_words, hipMemcpyDeviceToHost, c->stream));
    return drain.wait();
}

int scape_hip_report_perm_pairs(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                int32_t n_groups, const int32_t *seg_off, int32_t pair_first, int32_t pair_count,
                                int64_t *t_out, int64_t *a0_out, int64_t *site_n_ge_out, double *stat0_out,
                                int64_t *gene_n_ge_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    return rep_perm_ranged(
        c, s->pair_masks, "pair", (int32_t)(s->x_pairs.size() / 8), pair_first, pair_count, n_rec, rec_row_off, rows,
        n_groups, seg_off, t_out, a0_out, site_n_ge_out, stat0_out, gene_n_ge_out, k_rep_perm_pairs,
        [&](const RepPermCall &k) -> int { return rep_pair_segments(c, k, n_groups); },
        [&](const RepPermCall &k, const int32_t *recs, int64_t m, int32_t cap, size_t lds) {
            hipLaunchKernelGGL(k_rep_perm_pairs, dim3((uint32_t)(m * k.n_tiles), (uint32_t)pair_count), dim3(REP_THREADS),
                               lds, c->stream, s->x_bits.as<unsigned long long>(), k.p_count, k.n_tiles, recs,
                               s->p_roff.as<int64_t>(), s->x_seg.as<int64_t>(), s->p_nz.as<uint2>(),
                               s->q_a0.as<int64_t>(), n_groups, s->q_seg.as<int32_t>(),
                               s->x_desc.as<RepPair>() + pair_first, k.n_rows, n_rec, cap, s->p_site.as<int32_t>(),
                               s->p_gene.as<int32_t>(), s->p_stat0.as<double>());
        });
}

int scape_hip_report_perm_marker_masks(scape_hip_ctx *c, int32_t n_markers, const int32_t *sizes, int32_t n_others,
                                       const int32_t *orig_rank, int64_t p_first, int32_t p_count, uint64_t seed) {
    CTX_ENTER(c);
    if (n_markers < 1 || n_markers > REP_GROUPS_MAX)
        return fail("n_markers must lie in 1 .. " + std::to_string(REP_GROUPS_MAX));
    if (!sizes || !orig_rank) return fail("bad argument");
    if (rep_group_sizes_ok(n_markers, sizes)) return 1;
    if (n_others < 0) return fail("n_others must not be negative");
    std::vector<int32_t> seg((size_t)n_markers + 2, 0);      // the markers' segments, then the others'
    int64_t n = n_others;
    for (int32_t g = 0; g < n_markers; ++g) n += sizes[g];
    if (n < 2) return fail("the tested cells must number at least 2");
    if (rep_perm_chunk_ok(n, "the tested cells must number", p_first, p_count)) return 1;
    for (int32_t g = 0; g < n_markers; ++g) {
        if (sizes[g] >= n)
            return fail("marker " + std::to_string(g) + " holds every tested cell: its rest needs at least one");
        seg[(size_t)g + 1] = seg[g] + sizes[g];
    }
    seg[(size_t)n_markers + 1] = (int32_t)n;
    std::vector<bool> seen((size_t)n, false);
    for (int32_t g = 0; g <= n_markers; ++g)
        for (int32_t j = seg[g]; j < seg[(size_t)g + 1]; ++j) {
            const int32_t r = orig_rank[j];
            if (r < 0 || r >= n || seen[r]) return fail("orig_rank must be a permutation of 0 .. n - 1");
            seen[r] = true;
            if (j > seg[g] && r < orig_rank[j - 1]) return fail("orig_rank must ascend within every segment");
        }
    const int64_t n_words = (n + 63) / 64, words = n_words * n_markers;
    if (words > INT32_MAX) return fail("the markers' mask words together must number below 2^31");
    ReportState *s = report_state(c);
    s->marker_masks.count = 0;
    StreamDrain drain(c->stream);
    if (s->k_bits.ensure(words * p_count * 8) || s->k_bound.ensure((int64_t)n_markers * p_count * 8) ||
        s->k_seg.ensure(((int64_t)n_markers + 2) * 4) || s->k_rank.ensure(n * 4))
        return 1;
    HIPCHK(hipMemcpyAsync(s->k_seg.p, seg.data(), ((int64_t)n_markers + 2) * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->k_rank.p, orig_rank, n * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_rep_perm_marker_masks, dim3(p_count, n_markers), dim3(REP_THREADS), 0, c->stream,
                       s->k_seg.as<int32_t>(), s->k_rank.as<int32_t>(), (int32_t)n, (unsigned long long)p_first, p_count,
                       (unsigned long long)seed, s->k_bound.as<unsigned long long>(),
                       s->k_bits.as<unsigned long long>());
    s->marker_masks.sizes.assign(sizes, sizes + n_markers);
    s->marker_masks.sizes.push_back(n_others);
    return rep_built(drain, s->marker_masks, n, p_count);
}

int scape_hip_report_perm_marker_bits_get(scape_hip_ctx *c, int32_t marker, int32_t p, uint64_t *words_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    const RepLabellings &l = s->marker_masks;
    const bool marker_ok = marker >= 0 && marker < (int32_t)l.sizes.size() - 1;
    if (rep_get_ok(l, words_out, marker_ok ? nullptr : "marker must name a marker of the last marker masks call", p))
        return 1;
    const int64_t n_words = ((int64_t)l.n + 63) / 64;
    StreamDrain drain(c->stream);
    HIPCHK(hipMemcpy2DAsync(words_out, 8, s->k_bits.as<unsigned long long>() + marker * n_words * l.count + p,
                            (size_t)l.count * 8, 8, (size_t)n_words, hipMemcpyDeviceToHost, c->stream));
    return drain.wait();
}

int scape_hip_report_perm_markers(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                  int32_t n_seg, const int32_t *seg_off, int32_t marker_first, int32_t marker_count,
                                  int64_t *t_out, int64_t *a0_out, int64_t *site_n_ge_out, double *stat0_out,
                                  int64_t *gene_n_ge_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    return rep_perm_ranged(
        c, s->marker_masks, "marker", n_seg - 1, marker_first, marker_count, n_rec, rec_row_off, rows, n_seg, seg_off,
        t_out, a0_out, site_n_ge_out, stat0_out, gene_n_ge_out, k_rep_perm_markers,
        [](const RepPermCall &) -> int { return 0; },
        [&](const RepPermCall &k, const int32_t *recs, int64_t m, int32_t cap, size_t lds) {
            hipLaunchKernelGGL(k_rep_perm_markers, dim3((uint32_t)(m * k.n_tiles), (uint32_t)marker_count),
                               dim3(REP_THREADS), lds, c->stream, s->k_bits.as<unsigned long long>(), k.p_count,
                               k.n_tiles, (k.n + 63) / 64, recs, s->p_roff.as<int64_t>(), s->p_noff.as<int64_t>(),
                               s->p_nz.as<uint2>(), s->p_t.as<int64_t>(), s->q_a0.as<int64_t>(), n_seg, marker_first,
                               k.n_rows, n_rec, cap, s->p_site.as<int32_t>(), s->p_gene.as<int32_t>(),
                               s->p_stat0.as<double>());
        });
}

int scape_hip_report_perm_len_pairs(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                    int32_t n_groups, const int32_t *seg_off, int32_t pair_first, int32_t pair_count,
                                    const double *x, int64_t *t_out, int64_t *a0_out, double *delta0_out,
                                    int64_t *n_ge_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    return rep_perm_len_ranged(
        c, s->pair_masks, "pair", (int32_t)(s->x_pairs.size() / 8), pair_first, pair_count, n_rec, rec_row_off, rows,
        n_groups, seg_off, x, t_out, a0_out, delta0_out, n_ge_out,
        [&](const RepPermCall &k) -> int { return rep_pair_segments(c, k, n_groups); },
        [&](const RepPermCall &k) {
            hipLaunchKernelGGL(k_rep_perm_len_pairs, dim3((uint32_t)((int64_t)n_rec * k.n_tiles), (uint32_t)pair_count),
                               dim3(REP_THREADS), 0, c->stream, s->x_bits.as<unsigned long long>(), k.p_count, k.n_tiles,
                               s->p_roff.as<int64_t>(), s->x_seg.as<int64_t>(), s->p_nz.as<uint2>(),
                               s->q_a0.as<int64_t>(), n_groups, s->q_seg.as<int32_t>(),
                               s->x_desc.as<RepPair>() + pair_first, s->l_w.as<double>(), n_rec,
                               s->p_gene.as<int32_t>(), s->p_stat0.as<double>());
        });
}

int scape_hip_report_perm_len_markers(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                      int32_t n_seg, const int32_t *seg_off, int32_t marker_first, int32_t marker_count,
                                      const double *x, int64_t *t_out, int64_t *a0_out, double *delta0_out,
                                      int64_t *n_ge_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    return rep_perm_len_ranged(
        c, s->marker_masks, "marker", n_seg - 1, marker_first, marker_count, n_rec, rec_row_off, rows, n_seg, seg_off, x,
        t_out, a0_out, delta0_out, n_ge_out, [](const RepPermCall &) -> int { return 0; },
        [&](const RepPermCall &k) {
            hipLaunchKernelGGL(k_rep_perm_len_markers,
                               dim3((uint32_t)((int64_t)n_rec * k.n_tiles), (uint32_t)marker_count), dim3(REP_THREADS), 0,
                               c->stream, s->k_bits.as<unsigned long long>(), k.p_count, k.n_tiles, (k.n + 63) / 64,
                               s->p_roff.as<int64_t>(), s->p_noff.as<int64_t>(), s->p_nz.as<uint2>(),
                               s->p_t.as<int64_t>(), s->q_a0.as<int64_t>(), n_seg, marker_first, s->l_w.as<double>(),
                               n_rec, s->p_gene.as<int32_t>(), s->p_stat0.as<double>());
        });
}

int scape_hip_report_perm_scores(scape_hip_ctx *c, int32_t n, const uint16_t *q, int64_t p_first, int32_t p_count,
                                 uint64_t seed) {
    CTX_ENTER(c);
    if (!q) return fail("bad argument");
    if (n < 2) return fail("the scored cells must number 2 or more");
    if (rep_perm_chunk_ok(n, "the scored cells must number", p_first, p_count)) return 1;
    int32_t qspan = 0;
    for (int32_t j = 0; j < n; ++j) {
        if (q[j] > REP_SCORE_MAX) return fail("position " + std::to_string(j) + ": scores must lie in 0 .. 32,768");
        qspan = std::max<int32_t>(qspan, q[j]);
    }
    ReportState *s = report_state(c);
    s->scores.count = 0;
    StreamDrain drain(c->stream);
    int32_t bits = 0;                        // B = 2^bits: the smallest power of two that reaches n, within the limits
    while ((1 << bits) < REP_SCORE_MIN_BUCKETS || ((1 << bits) < n && (1 << bits) < REP_SCORE_MAX_BUCKETS)) ++bits;
    // a halfword per (position, permutation), and one scratch slice of n int32 per permutation of the chunk
    if (s->t_scores.ensure((int64_t)p_count * n * 2) || s->t_members.ensure((int64_t)p_count * n * 4) ||
        s->t_q.ensure((int64_t)n * 2))
        return 1;
    HIPCHK(hipMemcpyAsync(s->t_q.p, q, (int64_t)n * 2, hipMemcpyHostToDevice, c->stream));
    // the counters and, behind them, the four waves' sums of the scan: 16 bytes above 64 KiB at the most buckets
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_rep_perm_scores),
                               hipFuncAttributeMaxDynamicSharedMemorySize, REP_SCORE_MAX_BUCKETS * 4 + REP_WAVES * 4));
    hipLaunchKernelGGL(k_rep_perm_scores, dim3(p_count), dim3(REP_THREADS), ((size_t)4 << bits) + REP_WAVES * 4, c->stream, n, bits,
                       s->t_q.as<uint16_t>(), (unsigned long long)p_first, p_count, (unsigned long long)seed,
                       s->t_members.as<int32_t>(), s->t_scores.as<uint16_t>());
    s->t_qspan = qspan;
    return rep_built(drain, s->scores, n, p_count);
}

int scape_hip_report_perm_scores_get(scape_hip_ctx *c, int32_t p, uint16_t *scores_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    const RepLabellings &l = s->scores;
    if (rep_get_ok(l, scores_out, nullptr, p)) return 1;
    StreamDrain drain(c->stream);
    // the builder's scratch (4 n bytes per permutation) is idle between two scores calls: the column is gathered there
    hipLaunchKernelGGL(k_rep_scores_column, dim3((uint32_t)((l.n + REP_THREADS - 1) / REP_THREADS)), dim3(REP_THREADS),
                       0, c->stream, s->t_scores.as<uint16_t>(), l.n, l.count, p, s->t_members.as<uint16_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(scores_out, s->t_members.p, (int64_t)l.n * 2, hipMemcpyDeviceToHost, c->stream));
    return drain.wait();
}

int scape_hip_report_perm_trend(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                int64_t *t_out, int64_t *s0_out, int64_t *sq0_out, int64_t *site_n_ge_out,
                                double *d0_out, double *stat0_out, int64_t *gene_n_ge_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    if (s->scores.ready(s->n_cnt_rows)) return 1;
    RepPermCall k(c, s->scores, n_rec, rec_row_off, rows, t_out);
    k.outs_ok = s0_out && sq0_out && site_n_ge_out && d0_out && stat0_out && gene_n_ge_out;
    k.max_rec_rows = REP_TREND_MAX_ROWS;
    if (rep_trend_prepare(c, k)) return 1;
    const int64_t n_rows = k.n_rows;
    if (s->t_s0.ensure(n_rows * 8) || s->t_sq0.ensure(n_rows * 8) || s->v_qt.ensure((int64_t)n_rec * 16) ||
        s->v_tol.ensure((int64_t)n_rec * 16) || s->v_d0.ensure(n_rows * 8))
        return 1;
    return rep_perm_count(c, k, n_rows, n_rec, site_n_ge_out, gene_n_ge_out, stat0_out, [&]() -> int {
        hipLaunchKernelGGL(k_rep_trend_obs, dim3((uint32_t)n_rec), dim3(REP_THREADS), 0, c->stream,
                           s->p_roff.as<int64_t>(), s->p_noff.as<int64_t>(), s->p_nz.as<uint2>(), s->p_t.as<int64_t>(),
                           s->t_q.as<uint16_t>(), s->t_qspan, s->t_s0.as<long long>(), s->t_sq0.as<long long>(),
                           s->v_qt.as<long long>(), s->v_tol.as<double>(), s->v_d0.as<double>(),
                           s->p_stat0.as<double>());
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_rep_perm_trend, dim3((uint32_t)((int64_t)n_rec * k.n_tiles)), dim3(REP_THREADS), 0,
                           c->stream, s->t_scores.as<uint16_t>(), k.p_count, k.n_tiles, s->p_roff.as<int64_t>(),
                           s->p_noff.as<int64_t>(), s->p_nz.as<uint2>(), s->p_t.as<int64_t>(), s->v_qt.as<long long>(),
                           s->v_tol.as<double>(), s->v_d0.as<double>(), s->p_stat0.as<double>(),
                           s->p_site.as<int32_t>(), s->p_gene.as<int32_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(s0_out, s->t_s0.p, n_rows * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(sq0_out, s->t_sq0.p, n_rows * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(d0_out, s->v_d0.p, n_rows * 8, hipMemcpyDeviceToHost, c->stream));
        return 0;
    });
}

int scape_hip_report_perm_len_trend(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                    const int32_t *x, int64_t *t_out, int64_t *s0_out, int64_t *sq0_out,
                                    int64_t *c0_out, int64_t *n_ge_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    if (s->scores.ready(s->n_cnt_rows)) return 1;
    RepPermCall k(c, s->scores, n_rec, rec_row_off, rows, t_out);
    k.q = x, k.outs_ok = x && s0_out && sq0_out && c0_out && n_ge_out;
    if (rep_trend_prepare(c, k)) return 1;
    // T < 2^31 holds (rep_perm_prepare); T max x < 2^48 keeps Sxz, at scores of up to 2^15, below 2^63
    for (int r = 0; r < n_rec; ++r) {
        int64_t T = 0, max_x = 0;
        for (int64_t i = rec_row_off[r]; i < rec_row_off[r + 1]; ++i) {
            T += t_out[i];
            max_x = std::max<int64_t>(max_x, x[i]);
        }
        if (T * max_x >= REP_LEN_TREND_MAX_TX)
            return fail("record " + std::to_string(r) + ": reads x largest position must stay below 2^48");
    }
    const int64_t n_rows = k.n_rows;
    if (s->t_s0.ensure(n_rows * 8) || s->t_sq0.ensure(n_rows * 8) || s->v_q.ensure(n_rows * 4) ||
        s->t_lrec.ensure((int64_t)n_rec * REP_LEN_TREND_REC * 8))
        return 1;
    std::vector<int64_t> &rec = k.lrec;               // T, Sx, Sz(0), Sxz(0) and the halves of C(0) per record
    rec.resize((size_t)n_rec * REP_LEN_TREND_REC);
    if (rep_perm_count(c, k, 0, n_rec, nullptr, n_ge_out, nullptr, [&]() -> int {
            HIPCHK(hipMemcpyAsync(s->v_q.p, x, n_rows * 4, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_rep_len_trend_obs, dim3((uint32_t)n_rec), dim3(REP_THREADS), 0, c->stream,
                               s->p_roff.as<int64_t>(), s->p_noff.as<int64_t>(), s->p_nz.as<uint2>(),
                               s->p_t.as<int64_t>(), s->v_q.as<int32_t>(), s->t_q.as<uint16_t>(),
                               s->t_s0.as<long long>(), s->t_sq0.as<long long>(), s->t_lrec.as<long long>());
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_rep_perm_len_trend, dim3((uint32_t)((int64_t)n_rec * k.n_tiles)), dim3(REP_THREADS), 0,
                               c->stream, s->t_scores.as<uint16_t>(), k.p_count, k.n_tiles, s->p_roff.as<int64_t>(),
                               s->p_noff.as<int64_t>(), s->p_nz.as<uint2>(), s->v_q.as<int32_t>(),
                               s->t_lrec.as<long long>(), s->p_gene.as<int32_t>());
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(s0_out, s->t_s0.p, n_rows * 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(sq0_out, s->t_sq0.p, n_rows * 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(rec.data(), s->t_lrec.p, (int64_t)n_rec * REP_LEN_TREND_REC * 8, hipMemcpyDeviceToHost,
                                  c->stream));
            return 0;
        }))
        return 1;
    for (int r = 0; r < n_rec; ++r) {
        c0_out[2 * (size_t)r] = rec[(size_t)r * REP_LEN_TREND_REC + 4];
        c0_out[2 * (size_t)r + 1] = rec[(size_t)r * REP_LEN_TREND_REC + 5];
    }
    return 0;
}

}  // extern "C"

// ---- boot_pa_len: the cell bootstrap of the mean pA position per population -------------------------------------------
// Percentile intervals of a record's mean pA position in each of G = 1..64 populations, by resampling the cells (the
// Poisson bootstrap).  The tested columns are the populations' columns in front of the count matrix, population 0's
// first: position j = column j, in the column segments seg_off, and position j carries cell[j], the 0-based column its
// cell has in ex_pa_cnt_mat's matrix.  The hash sees cell[j], not j: a cell's multiplicity does not depend on the
// clustering.  All arithmetic mod 2^64, G and mix those of scape_hip_report_perm_masks:
//   h(b, c) = mix(mix(seed + G b) + G (c + 1)),  all 64 bits
//   m(b, c) = #{k in 0..14 : h(b, c) >= P[k]}  for replicate b >= 1, so 0 <= m <= 15;  replicate 0 is the observed data, m = 1
//   P[k] = floor(2^64 e^-1 sum_{i <= k} 1 / i!):  m is Poisson(1), its tail beyond 15 (1.9e-14) folded into m = 15
// Kept row i of a record carries the integer position q_i, 0 <= q_i <= 2^22; with c_ij its count at position j and g(j)
// the population of position j:
//   A_g(b) = sum_i sum_{j in g} m(b, cell[j]) c_ij,   Q_g(b) = sum_i q_i sum_{j in g} m(b, cell[j]) c_ij
// are exact integers whatever the order of the adds: a record has T < 2^27 reads in the tested cells (checked), so
// A <= 15 T < 2^31 and Q <= 15 T 2^22 < 2^53.  The replicate's value is
//   v_g(b) = (double)Q_g(b) / (double)A_g(b),  one IEEE division, contraction off;  +infinity when A_g(b) = 0.
// Every defined value lies in 0 .. 2^22, so the values' bit patterns, read as unsigned 64-bit integers, order as the
// values do, with +infinity last.  Per series (record, population), over the replicates 1 .. n_boot and a level of L
// basis points:
//   D = #{b : A_g(b) > 0},  k = max(1, floor((D + 1) (10000 - L) / 20000)) in integers,
//   lo = the k-th smallest of the n_boot values,  hi = the (D + 1 - k)-th smallest;  both +infinity when D = 0.
//   k_rep_boot_mult    elementwise: lanes along the replicates (the byte stores of one position are contiguous), the
//                      replicate's inner hash base formed once per lane, the 15 comparisons added up
//   k_rep_boot_len     workgroup = (record, tile of 256 replicates), one lane per replicate.  A nonzero's population is
//                      fixed by its column segment, so the walk goes population by population over the row's nonzeros of
//                      that segment (k_rep_pair_segidx found where they start): A and Q of the one population live in
//                      registers, every nonzero is read once, and there is no LDS, no atomic, no barrier and no slice
//   k_rep_boot_select  one workgroup per series: D by a count, then a radix select over the bit patterns (through the
//                      key below, which keeps this order), most significant byte first, both ranks in the same eight
//                      passes over the series (which stays in L2)
// boot_pa_usage, on the same multiplicities: with a_ig(b) = sum_{j in g} m(b, cell[j]) c_ij and A_g(b) = sum_i a_ig(b),
//   u_ig(b) = (double)a_ig(b) / (double)A_g(b),  one IEEE division, contraction off;  +infinity when A_g(b) = 0
// per series (kept row i, population g).  Every defined value lies in 0 .. 1, so the bit patterns order as above and D,
// k, lo and hi are the same rule by the same k_rep_boot_select.
//   k_rep_boot_usage   workgroup and lanes of k_rep_boot_len; per population the a_ig of a record of up to 8 kept rows
//                      from one walk, held in registers until A_g is known; of a longer record A_g by a walk over all
//                      its rows, then a_ig row by row; the quotients stored along the replicates; no LDS, atomic or
//                      barrier
// boot_pa_len_diff and boot_pa_usage_diff, for exactly two populations (segment 0 minus segment 1), one series per
// record or per kept row:
//   d(b)   = (double)Q_1(b) / (double)A_1(b) - (double)Q_2(b) / (double)A_2(b)
//   d_i(b) = (double)a_i1(b) / (double)A_1(b) - (double)a_i2(b) / (double)A_2(b)
// two IEEE divisions and one IEEE subtraction, contraction off: the v_g and u_ig above, subtracted;  +infinity when
// A_1(b) = 0 or A_2(b) = 0.  A difference may be negative, so the select orders keys, not bit patterns:
//   key(x) = bits(x) ^ (bits(x) >> 63 ? ~0 : 1 << 63)
// is monotone over the finite doubles and puts +infinity above them all; "defined" is key < key(+infinity) and the result
// is the inverse map of the selected key.  Over non-negative values the keys order as the bit patterns do, so boot_len's
// and boot_usage's record sets go through the same select and get the bits they always got.  -0.0 (whose key lies below
// that of +0.0) cannot occur: a quotient of non-negative integers is never -0, and x - x is +0.0 under round-to-nearest.
//   k_rep_boot_len_diff    k_rep_boot_len's body with both populations in one series; A_1, Q_1, A_2, Q_2 in registers,
//                          one walk of every kept row's nonzeros, segment 0 into population 1's sums and segment 1 into
//                          population 2's
//   k_rep_boot_usage_diff  k_rep_boot_usage's body likewise, in its two shapes: up to 8 kept rows, one walk per
//                          population with a_i1 and a_i2 in registers; more, A_1 and A_2 by a first walk and then row by
//                          row
#define REP_BOOT_READS_BITS 27         // T < 2^27
#define REP_BOOT_MULT_POS 64           // positions a workgroup of k_rep_boot_mult takes per step
#define REP_BOOT_USAGE_REG_ROWS 8      // kept rows of a record up to which k_rep_boot_usage holds every a_ig in a register

__device__ __forceinline__ int rep_boot_mult(unsigned long long h) {
    constexpr unsigned long long P[15] = {
        0x5E2D58D8B3BCDF1Aull, 0xBC5AB1B16779BE35ull, 0xEB715E1DC1582DC2ull, 0xFB23979734A252F1ull, 0xFF1025F59174DC3Dull,
        0xFFD90F3BA4055E19ull, 0xFFFA8B71FC72C913ull, 0xFFFF540C0914B3C9ull, 0xFFFFED1F4AA8F120ull, 0xFFFFFE216E641462ull,
        0xFFFFFFD4D85D3183ull, 0xFFFFFFFC6DA262B4ull, 0xFFFFFFFFBA12D178ull, 0xFFFFFFFFFB07C64Cull, 0xFFFFFFFFFFAB8EA5ull};
    int m = 0;
#pragma unroll
    for (int k = 0; k < 15; ++k) m += h >= P[k];
    return m;
}

// workgroup = (tile of 256 replicates blockIdx.x, positions blockIdx.y * 64 .. in steps of gridDim.y * 64): lane = the
// replicate b_first + tile * 256 + threadIdx.x, cell[j] is wave-uniform
__global__ __launch_bounds__(REP_THREADS) void k_rep_boot_mult(int32_t n, const int32_t *__restrict__ cell,
                                                               unsigned long long b_first, int32_t b_count,
                                                               unsigned long long seed, uint8_t *__restrict__ mult) {
    const int p = blockIdx.x * REP_THREADS + threadIdx.x;
    if (p >= b_count) return;
    const unsigned long long base = rep_mix(seed + REP_PERM_G * (b_first + (unsigned long long)p));
    for (int j0 = blockIdx.y * REP_BOOT_MULT_POS; j0 < n; j0 += gridDim.y * REP_BOOT_MULT_POS) {
        const int j1 = min(n, j0 + REP_BOOT_MULT_POS);
        for (int j = j0; j < j1; ++j) {
            const unsigned long long c = (unsigned long long)cell[j];
            mult[(int64_t)j * b_count + p] = (uint8_t)rep_boot_mult(rep_mix(base + REP_PERM_G * (c + 1)));
        }
    }
}

// The value kernels.  workgroup = (record blockIdx.x / n_tiles, tile of 256 replicates of the chunk), one lane per
// replicate; a lane beyond the chunk walks the last replicate's bytes and stores nothing.  sg[i] = the n_groups + 1 segment
// starts of kept row i among the nonzeros.  A series covers NB populations: one (its value is that population's quotient)
// or the two of a difference (population 0's quotient minus population 1's); its values lie at
// vals[series * n_boot + col0 + replicate of the chunk], stored along the replicates
struct RepBootLane {
    int r, p;                    // record; replicate of the chunk
    bool valid;
    const uint8_t *mb;           // the replicate's multiplicity of position 0
    int64_t row0, row1;          // the record's kept rows
};

__device__ __forceinline__ RepBootLane rep_boot_lane(const uint8_t *__restrict__ mult, int32_t b_count, int32_t n_tiles,
                                                     const int64_t *__restrict__ roff) {
    RepBootLane l;
    l.r = blockIdx.x / n_tiles;
    l.p = (blockIdx.x % n_tiles) * REP_THREADS + threadIdx.x;
    l.valid = l.p < b_count;
    l.mb = mult + (l.valid ? l.p : b_count - 1);
    l.row0 = roff[l.r], l.row1 = roff[l.r + 1];
    return l;
}

// a_ig: the sum of m x c over the nonzeros of kept row i in segment g (m <= 15 and the row's reads stay below 2^27)
__device__ __forceinline__ int rep_boot_row_sum(const uint2 *__restrict__ nz, const int64_t *__restrict__ sg, int n_groups,
                                                int64_t i, int g, const uint8_t *__restrict__ mb, int32_t b_count) {
    const int64_t *si = sg + i * (n_groups + 1);
    int a = 0;
    rep_groups_walk(nz, si[g], si[g + 1], mb, b_count, [&](int m, int c) { a += m * c; });
    return a;
}

// a series' value from the num / den of its NB populations
template <int NB, typename T>
__device__ __forceinline__ double rep_boot_value(const T *num, const T *den) {
#pragma clang fp contract(off)
    if (NB == 1) return den[0] > 0 ? (double)num[0] / (double)den[0] : __builtin_huge_val();
    return den[0] > 0 && den[NB - 1] > 0 ? (double)num[0] / (double)den[0] - (double)num[NB - 1] / (double)den[NB - 1]
                                         : __builtin_huge_val();
}

// v_g = Q_g / A_g: one series per record and NB populations.  The walk takes the populations NB at a time, per kept row
// the row's nonzeros of those segments (k_rep_pair_segidx found where they start): A and Q live in registers, every
// nonzero is read once, and there is no LDS, no atomic, no barrier and no slice
template <int NB>
__device__ __forceinline__ void rep_boot_len_body(const uint8_t *__restrict__ mult, int32_t b_count, int32_t n_tiles,
                                                  int32_t n_groups, const int64_t *__restrict__ roff,
                                                  const int64_t *__restrict__ sg, const uint2 *__restrict__ nz,
                                                  const int32_t *__restrict__ q, int64_t n_boot, int64_t col0,
                                                  double *__restrict__ vals) {
    const RepBootLane l = rep_boot_lane(mult, b_count, n_tiles, roff);
    for (int g0 = 0; g0 < n_groups; g0 += NB) {
        long long A[NB] = {}, Q[NB] = {};
        for (int64_t i = l.row0; i < l.row1; ++i) {
            int a[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) a[b] = rep_boot_row_sum(nz, sg, n_groups, i, g0 + b, l.mb, b_count);
            const long long qi = q[i];
#pragma unroll
            for (int b = 0; b < NB; ++b) A[b] += a[b], Q[b] += a[b] * qi;
        }
        if (l.valid)
            vals[((int64_t)l.r * (n_groups / NB) + g0 / NB) * n_boot + col0 + l.p] = rep_boot_value<NB>(Q, A);
    }
}

// u_ig = a_ig / A_g: one series per kept row i of the call (not the record) and NB populations.  15 T < 2^31: both sums
// are 32-bit.  A record of at most REP_BOOT_USAGE_REG_ROWS kept rows takes one walk per population, the a_ig of its rows
// in registers until A_g is known (the branch is uniform over the workgroup and taken once, in front of the
// populations); a longer one takes two: A_g over all its rows, then a_ig row by row, which finds the multiplicity bytes
// of the first walk in cache.  Measured at records of 2..8 rows: 32.9 ms with the one walk, 50.3 ms with two walks for
// every record.  No LDS, atomic or barrier
template <int NB>
__device__ __forceinline__ void rep_boot_usage_body(const uint8_t *__restrict__ mult, int32_t b_count, int32_t n_tiles,
                                                    int32_t n_groups, const int64_t *__restrict__ roff,
                                                    const int64_t *__restrict__ sg, const uint2 *__restrict__ nz,
                                                    const int32_t *__restrict__, int64_t n_boot, int64_t col0,
                                                    double *__restrict__ vals) {
    const RepBootLane l = rep_boot_lane(mult, b_count, n_tiles, roff);
    const int n_series = n_groups / NB;          // per kept row
    if (l.row1 - l.row0 <= REP_BOOT_USAGE_REG_ROWS) {
        for (int g0 = 0; g0 < n_groups; g0 += NB) {
            int a[REP_BOOT_USAGE_REG_ROWS][NB], A[NB] = {};
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int k = 0; k < REP_BOOT_USAGE_REG_ROWS; ++k) {
                    a[k][b] = 0;
                    if (l.row0 + k < l.row1) {
                        a[k][b] = rep_boot_row_sum(nz, sg, n_groups, l.row0 + k, g0 + b, l.mb, b_count);
                        A[b] += a[k][b];
                    }
                }
#pragma unroll
            for (int k = 0; k < REP_BOOT_USAGE_REG_ROWS; ++k)
                if (l.row0 + k < l.row1 && l.valid)
                    vals[((l.row0 + k) * n_series + g0 / NB) * n_boot + col0 + l.p] = rep_boot_value<NB>(a[k], A);
        }
        return;
    }
    for (int g0 = 0; g0 < n_groups; g0 += NB) {
        int A[NB] = {};
        for (int64_t i = l.row0; i < l.row1; ++i)
#pragma unroll
            for (int b = 0; b < NB; ++b) A[b] += rep_boot_row_sum(nz, sg, n_groups, i, g0 + b, l.mb, b_count);
        for (int64_t i = l.row0; i < l.row1; ++i) {
            int a[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) a[b] = rep_boot_row_sum(nz, sg, n_groups, i, g0 + b, l.mb, b_count);
            if (l.valid) vals[(i * n_series + g0 / NB) * n_boot + col0 + l.p] = rep_boot_value<NB>(a, A);
        }
    }
}

// the four kernels, under the names the kernel traces know, on one parameter list: the differences get n_groups = 2,
// the usage kernels no q.  The usage kernels' bound asks for 8 waves per SIMD: as a body behind a wrapper the register
// path takes 106 scalar registers and 7 waves without it (the same text as a kernel of its own: 100 and 8), 78 and 8
// with it, and with it the two kernels are 7 to 19 % faster than before the fold in both paths; the length kernels have
// 8 waves unasked and were 1.1 to 1.5 % slower under the bound (profiles/boot_one_body_timing.txt)
__global__ __launch_bounds__(REP_THREADS) void k_rep_boot_len(
    const uint8_t *__restrict__ mult, int32_t b_count, int32_t n_tiles, int32_t n_groups,
    const int64_t *__restrict__ roff, const int64_t *__restrict__ sg, const uint2 *__restrict__ nz,
    const int32_t *__restrict__ q, int64_t n_boot, int64_t col0, double *__restrict__ vals) {
    rep_boot_len_body<1>(mult, b_count, n_tiles, n_groups, roff, sg, nz, q, n_boot, col0, vals);
}

__global__ __launch_bounds__(REP_THREADS, 8) void k_rep_boot_usage(
    const uint8_t *__restrict__ mult, int32_t b_count, int32_t n_tiles, int32_t n_groups,
    const int64_t *__restrict__ roff, const int64_t *__restrict__ sg, const uint2 *__restrict__ nz,
    const int32_t *__restrict__ q, int64_t n_boot, int64_t col0, double *__restrict__ vals) {
    rep_boot_usage_body<1>(mult, b_count, n_tiles, n_groups, roff, sg, nz, q, n_boot, col0, vals);
}

__global__ __launch_bounds__(REP_THREADS) void k_rep_boot_len_diff(
    const uint8_t *__restrict__ mult, int32_t b_count, int32_t n_tiles, int32_t n_groups,
    const int64_t *__restrict__ roff, const int64_t *__restrict__ sg, const uint2 *__restrict__ nz,
    const int32_t *__restrict__ q, int64_t n_boot, int64_t col0, double *__restrict__ vals) {
    rep_boot_len_body<2>(mult, b_count, n_tiles, n_groups, roff, sg, nz, q, n_boot, col0, vals);
}

__global__ __launch_bounds__(REP_THREADS, 8) void k_rep_boot_usage_diff(
    const uint8_t *__restrict__ mult, int32_t b_count, int32_t n_tiles, int32_t n_groups,
    const int64_t *__restrict__ roff, const int64_t *__restrict__ sg, const uint2 *__restrict__ nz,
    const int32_t *__restrict__ q, int64_t n_boot, int64_t col0, double *__restrict__ vals) {
    rep_boot_usage_body<2>(mult, b_count, n_tiles, n_groups, roff, sg, nz, q, n_boot, col0, vals);
}

// the select's order: monotone over the finite doubles of either sign, +infinity above them all
__device__ __forceinline__ unsigned long long rep_boot_key(unsigned long long bits) {
    return bits ^ (bits >> 63 ? ~0ull : 1ull << 63);
}

__device__ __forceinline__ unsigned long long rep_boot_unkey(unsigned long long key) {
    return key ^ (key >> 63 ? 1ull << 63 : ~0ull);
}

struct RepBootSelectLds {
    __align__(16) int hist[2][256];
    unsigned long long sel[2];        // per rank looked for: the prefix of its value's key
    long long rank[2];                // and its rank among the values that share the prefix
    int defined;
};

// one workgroup per series: n_def[series] = D; lo[series], hi[series] by the rule above, over the keys of the values.
// Values tie, so the select takes all eight bytes; wave w < 2 finds the bin of rank w
__global__ __launch_bounds__(REP_THREADS) void k_rep_boot_select(const unsigned long long *__restrict__ vals,
                                                                 int64_t n_boot, int32_t level_bp,
                                                                 double *__restrict__ lo, double *__restrict__ hi,
                                                                 int64_t *__restrict__ n_def) {
    __shared__ RepBootSelectLds lds;
    const unsigned long long *v = vals + (int64_t)blockIdx.x * n_boot;
    const unsigned long long inf_key = rep_boot_key(0x7FF0000000000000ull);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) lds.defined = 0;
    __syncthreads();
    int mine = 0;
    for (int64_t i = threadIdx.x; i < n_boot; i += REP_THREADS) mine += rep_boot_key(v[i]) < inf_key;
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0 && mine) atomicAdd(&lds.defined, mine);
    __syncthreads();
    const long long D = lds.defined;
    if (D == 0) {
        if (threadIdx.x == 0) {
            lo[blockIdx.x] = hi[blockIdx.x] = __builtin_huge_val();
            n_def[blockIdx.x] = 0;
        }
        return;
    }
    long long k = (D + 1) * (10000 - level_bp) / 20000;
    if (k < 1) k = 1;
    unsigned long long prefix[2] = {0, 0};
    long long rank[2] = {k - 1, D - k};      // 0-based; both below D, so both values are defined
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        lds.hist[0][threadIdx.x] = 0;
        lds.hist[1][threadIdx.x] = 0;
        __syncthreads();
        for (int64_t i = threadIdx.x; i < n_boot; i += REP_THREADS) {
            const unsigned long long x = rep_boot_key(v[i]);
#pragma unroll
            for (int w = 0; w < 2; ++w)
                if (pass == 0 || (x >> (shift + 8)) == (prefix[w] >> (shift + 8)))
                    atomicAdd(&lds.hist[w][(x >> shift) & 255], 1);
        }
        __syncthreads();
        if (wave < 2) {                      // the bin that holds the value of that rank
            const int4 h = reinterpret_cast<const int4 *>(lds.hist[wave])[lane];
            const long long sum = (long long)h.x + h.y + h.z + h.w;
            long long incl = sum;
            for (int o = 1; o < 64; o <<= 1) {
                const long long y = __shfl_up(incl, o, 64);
                if (lane >= o) incl += y;
            }
            const long long want = rank[wave];
            if (incl - sum <= want && want < incl) {         // one lane: the bins are disjoint
                long long rr = want - (incl - sum);
                int b = 4 * lane;
                if (rr >= h.x) {
                    rr -= h.x, ++b;
                    if (rr >= h.y) {
                        rr -= h.y, ++b;
                        if (rr >= h.z) rr -= h.z, ++b;
                    }
                }
                lds.sel[wave] = prefix[wave] | ((unsigned long long)b << shift);
                lds.rank[wave] = rr;
            }
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            prefix[w] = lds.sel[w];
            rank[w] = lds.rank[w];
        }
    }
    if (threadIdx.x == 0) {
        lo[blockIdx.x] = __longlong_as_double((long long)rep_boot_unkey(prefix[0]));
        hi[blockIdx.x] = __longlong_as_double((long long)rep_boot_unkey(prefix[1]));
        n_def[blockIdx.x] = D;
    }
}

// ---- boot_pa_len: host side -------------------------------------------------------------------------------------------
// a refused call names its entry point in front of the message
static int rep_boot_named(const char *entry, int rc) {
    if (rc) g_err = std::string(entry) + ": " + g_err;
    return rc;
}

static int rep_boot_build(scape_hip_ctx *c, int32_t n, const int32_t *cell, int64_t b_first, int32_t b_count,
                          uint64_t seed) {
    if (n < 1 || n >= REP_PERM_MAX_N) return fail("n must lie in 1 .. 2^24 - 1");
    if (!cell) return fail("bad argument");
    for (int32_t j = 0; j < n; ++j)
        if (cell[j] < 0) return fail("position " + std::to_string(j) + ": a negative cell");
    if (b_first < 1 || b_count < 1) return fail("b_first and b_count must be at least 1 (replicate 0 is the observed data)");
    ReportState *s = report_state(c);
    s->boot.count = 0;
    StreamDrain drain(c->stream);
    if (s->b_mult.ensure((int64_t)b_count * n) || s->b_cell.ensure((int64_t)n * 4)) return 1;
    HIPCHK(hipMemcpyAsync(s->b_cell.p, cell, (int64_t)n * 4, hipMemcpyHostToDevice, c->stream));
    const uint32_t n_tiles = (uint32_t)((b_count + REP_THREADS - 1) / REP_THREADS);
    const uint32_t n_pos = (uint32_t)std::min<int64_t>(((int64_t)n + REP_BOOT_MULT_POS - 1) / REP_BOOT_MULT_POS, 65535);
    hipLaunchKernelGGL(k_rep_boot_mult, dim3(n_tiles, n_pos), dim3(REP_THREADS), 0, c->stream, n, s->b_cell.as<int32_t>(),
                       (unsigned long long)b_first, b_count, (unsigned long long)seed, s->b_mult.as<uint8_t>());
    s->b_first = b_first;
    return rep_built(drain, s->boot, n, b_count);
}

// The frame of the four entry points that write replicate values, by the kind of their record set: scape_hip_report_
// boot_len (q = the rows' positions, one series per record and group), _boot_usage (no q, one series per kept row and
// group) and their differences _boot_len_diff and _boot_usage_diff (exactly two groups, one series per record or per
// kept row): the checks, the compaction with the segment starts, the values' array and its written columns, and the
// kind's kernel.  A record set is its first chunk's entry point's (b_kind): a later chunk through another one is
// refused
enum RepBootKind : int32_t { REP_BOOT_LEN, REP_BOOT_USAGE, REP_BOOT_LEN_DIFF, REP_BOOT_USAGE_DIFF };

static int rep_boot_values(scape_hip_ctx *c, RepBootKind kind, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                           int32_t n_groups, const int32_t *seg_off, const int32_t *q, int64_t n_boot, int64_t *t_out,
                           int64_t *a0_out) {
    static constexpr decltype(&k_rep_boot_len) kernels[] = {k_rep_boot_len, k_rep_boot_usage, k_rep_boot_len_diff,
                                                            k_rep_boot_usage_diff};
    ReportState *s = report_state(c);
    const RepLabellings &l = s->boot;
    if (l.ready(s->n_cnt_rows)) return 1;
    const bool usage = kind == REP_BOOT_USAGE || kind == REP_BOOT_USAGE_DIFF;
    const bool diff = kind == REP_BOOT_LEN_DIFF || kind == REP_BOOT_USAGE_DIFF;
    if (diff && n_groups != 2) return fail("n_groups must be 2: the difference is population 0 minus population 1");
    if (n_groups < 1 || n_groups > REP_GROUPS_MAX) return fail("n_groups must lie in 1 .. " + std::to_string(REP_GROUPS_MAX));
    if (!seg_off) return fail("bad argument");
    if (seg_off[0] != 0) return fail("seg_off must start at 0 (position j is column j)");
    for (int32_t g = 0; g < n_groups; ++g)
        if (seg_off[g + 1] < seg_off[g]) return fail("seg_off must be non-decreasing");
    if (seg_off[n_groups] != l.n) return fail("seg_off must end at the positions of the last " + std::string(l.builder) + " call");
    const int64_t b_first = s->b_first, b_count = l.count;
    if (n_boot < 1 || n_boot > INT32_MAX || b_first + b_count - 1 > n_boot)
        return fail("the replicates of the last " + std::string(l.builder) + " call must lie in 1 .. n_boot, and n_boot below 2^31");
    if (n_rec <= 0 || (usage && !rec_row_off)) return fail("bad argument");
    if (usage && (rec_row_off[n_rec] <= 0 || rec_row_off[n_rec] > INT32_MAX))
        return fail("rec_row_off must end at the row count, between 1 and 2^31 - 1");
    const int64_t n_series = (usage ? rec_row_off[n_rec] : (int64_t)n_rec) * (diff ? 1 : n_groups);
    if (b_first > 1 && (n_series != s->b_series || n_groups != s->b_groups || n_boot != s->b_n_boot || kind != s->b_kind))
        return fail("a later chunk of replicates needs the records, groups and n_boot of the call that began at replicate 1, "
                    "and its entry point");
    if (n_series > INT32_MAX || n_series > INT64_MAX / 8 / n_boot)
        return fail(std::string("too many ") + (usage ? "rows" : "records") + " x groups x replicates for one call");
    RepPermCall k(c, l, n_rec, rec_row_off, rows, t_out);
    k.a0_out = a0_out, k.n_groups = n_groups, k.seg_off = seg_off, k.q = q, k.outs_ok = usage || q != nullptr;
    k.reads_bits = REP_BOOT_READS_BITS;
    if (rep_perm_prepare(c, k)) return 1;
    if (rep_pair_segments(c, k, n_groups) || (q && s->b_q.ensure(k.n_rows * 4))) return 1;
    if (b_first == 1) {
        s->b_series = 0;                       // nothing to select from until this call has succeeded
        if (s->b_vals.ensure(n_series * n_boot * 8)) return 1;
        s->b_written.assign((size_t)n_boot, 0);
    }
    if (q) HIPCHK(hipMemcpyAsync(s->b_q.p, q, k.n_rows * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(kernels[kind], dim3((uint32_t)((int64_t)n_rec * k.n_tiles)), dim3(REP_THREADS), 0, c->stream,
                       s->b_mult.as<uint8_t>(), k.p_count, k.n_tiles, n_groups, s->p_roff.as<int64_t>(),
                       s->x_seg.as<int64_t>(), s->p_nz.as<uint2>(), q ? s->b_q.as<int32_t>() : nullptr, n_boot,
                       b_first - 1, s->b_vals.as<double>());
    HIPCHK(hipGetLastError());
    if (k.drain.wait()) return 1;
    s->b_series = n_series, s->b_groups = n_groups, s->b_n_boot = (int32_t)n_boot, s->b_kind = kind;
    std::fill(s->b_written.begin() + (b_first - 1), s->b_written.begin() + (b_first - 1 + b_count), 1);
    return 0;
}

// the replicate values are there: a boot_len or boot_usage call has succeeded since they were allocated
static int rep_boot_vals_ok(const ReportState *s) {
    return s->b_series ? 0 : fail("scape_hip_report_boot_usage or scape_hip_report_boot_len has not been called");
}

static int rep_boot_quantiles(scape_hip_ctx *c, int32_t level_bp, double *lo_out, double *hi_out, int64_t *n_def_out) {
    ReportState *s = report_state(c);
    if (rep_boot_vals_ok(s)) return 1;
    if (!lo_out || !hi_out || !n_def_out) return fail("bad argument");
    if (level_bp < 1 || level_bp > 9999) return fail("level_bp must lie in 1 .. 9999 (basis points)");
    for (size_t b = 0; b < s->b_written.size(); ++b)
        if (!s->b_written[b])
            return fail("replicate " + std::to_string(b + 1) + " has not been written since the values were allocated");
    const int64_t n_series = s->b_series;
    if (s->b_lo.ensure(n_series * 8) || s->b_hi.ensure(n_series * 8) || s->b_def.ensure(n_series * 8)) return 1;
    StreamDrain drain(c->stream);
    hipLaunchKernelGGL(k_rep_boot_select, dim3((uint32_t)n_series), dim3(REP_THREADS), 0, c->stream,
                       s->b_vals.as<unsigned long long>(), (int64_t)s->b_n_boot, level_bp, s->b_lo.as<double>(),
                       s->b_hi.as<double>(), s->b_def.as<int64_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(lo_out, s->b_lo.p, n_series * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(hi_out, s->b_hi.p, n_series * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(n_def_out, s->b_def.p, n_series * 8, hipMemcpyDeviceToHost, c->stream));
    return drain.wait();
}

extern "C" {

int scape_hip_report_boot_mult(scape_hip_ctx *c, int32_t n, const int32_t *cell, int64_t b_first, int32_t b_count,
                               uint64_t seed) {
    CTX_ENTER(c);
    return rep_boot_named("scape_hip_report_boot_mult", rep_boot_build(c, n, cell, b_first, b_count, seed));
}

int scape_hip_report_boot_mult_get(scape_hip_ctx *c, int32_t b, uint8_t *mult_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    const RepLabellings &l = s->boot;
    if (rep_get_ok(l, mult_out, nullptr, b)) return rep_boot_named("scape_hip_report_boot_mult_get", 1);
    StreamDrain drain(c->stream);
    HIPCHK(hipMemcpy2DAsync(mult_out, 1, s->b_mult.as<uint8_t>() + b, (size_t)l.count, 1, (size_t)l.n,
                            hipMemcpyDeviceToHost, c->stream));
    return drain.wait();
}

int scape_hip_report_boot_len(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                              int32_t n_groups, const int32_t *seg_off, const int32_t *q, int64_t n_boot, int64_t *t_out,
                              int64_t *a0_out) {
    CTX_ENTER(c);
    return rep_boot_named("scape_hip_report_boot_len",
                          rep_boot_values(c, REP_BOOT_LEN, n_rec, rec_row_off, rows, n_groups, seg_off, q, n_boot,
                                          t_out, a0_out));
}

int scape_hip_report_boot_usage(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                int32_t n_groups, const int32_t *seg_off, int64_t n_boot, int64_t *t_out,
                                int64_t *a0_out) {
    CTX_ENTER(c);
    return rep_boot_named("scape_hip_report_boot_usage",
                          rep_boot_values(c, REP_BOOT_USAGE, n_rec, rec_row_off, rows, n_groups, seg_off, nullptr,
                                          n_boot, t_out, a0_out));
}

int scape_hip_report_boot_len_diff(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                   int32_t n_groups, const int32_t *seg_off, const int32_t *q, int64_t n_boot,
                                   int64_t *t_out, int64_t *a0_out) {
    CTX_ENTER(c);
    return rep_boot_named("scape_hip_report_boot_len_diff",
                          rep_boot_values(c, REP_BOOT_LEN_DIFF, n_rec, rec_row_off, rows, n_groups, seg_off, q, n_boot,
                                          t_out, a0_out));
}

int scape_hip_report_boot_usage_diff(scape_hip_ctx *c, int32_t n_rec, const int64_t *rec_row_off, const int64_t *rows,
                                     int32_t n_groups, const int32_t *seg_off, int64_t n_boot, int64_t *t_out,
                                     int64_t *a0_out) {
    CTX_ENTER(c);
    return rep_boot_named("scape_hip_report_boot_usage_diff",
                          rep_boot_values(c, REP_BOOT_USAGE_DIFF, n_rec, rec_row_off, rows, n_groups, seg_off, nullptr,
                                          n_boot, t_out, a0_out));
}

int scape_hip_report_boot_vals_get(scape_hip_ctx *c, int64_t series, double *vals_out) {
    CTX_ENTER(c);
    ReportState *s = report_state(c);
    if (rep_boot_vals_ok(s)) return rep_boot_named("scape_hip_report_boot_vals_get", 1);
    if (!vals_out || series < 0 || series >= s->b_series)
        return rep_boot_named("scape_hip_report_boot_vals_get", fail("series must name a series of the last boot_len or boot_usage record set"));
    StreamDrain drain(c->stream);
    HIPCHK(hipMemcpyAsync(vals_out, s->b_vals.as<double>() + series * s->b_n_boot, (int64_t)s->b_n_boot * 8,
                          hipMemcpyDeviceToHost, c->stream));
    return drain.wait();
}

int scape_hip_report_boot_quantiles(scape_hip_ctx *c, int32_t level_bp, double *lo_out, double *hi_out,
                                    int64_t *n_def_out) {
    CTX_ENTER(c);
    return rep_boot_named("scape_hip_report_boot_quantiles", rep_boot_quantiles(c, level_bp, lo_out, hi_out, n_def_out));
}

}  // extern "C"
