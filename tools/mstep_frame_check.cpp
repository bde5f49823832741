// mstep_frame_check.cpp - host check of the frame the three M-step kernels share (mstep.inc; no GPU needed).
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined \
//         -o mstep_frame_check tools/mstep_frame_check.cpp && ./mstep_frame_check
// (main makes no HIP call; the sanitizers instrument the host side only.  Run it on the CPU.)
//
// The program includes the library's source, so it drives the very __host__ __device__ rules k2_mstep, k3_mstep and
// k4_mstep are built from, and compares them with plain restatements written here:
//   1. mstep_block: over the launch grid ((n_utr + 7) / 8) * 8 * extent, n_utr = 1..20, extent = 1..5, every live
//      (UTR, tile) pair is produced exactly once, every other block is rejected, and from 8 UTRs on all tiles of a UTR
//      fall on blocks of one residue mod 8 (one XCD);
//   2. the LDS swizzle: with the 1-KB pieces of a slot written lane-linear by lanes that fetch m3_src_unit, the f64
//      that m3_frag_index reads for (slot row 16 w + rc, bin 4 s + kq) is that row's bin, for tile rows (w = wavefront)
//      and, on a job-vector slot written by k4_mstep's two vector wavefronts (k3_mstep's pieces land in the same
//      places), for job slots (w = column group), and the 16 rows x 2 taps of one fragment read hit 32 distinct
//      8-byte bank pairs;
//   3. mstep_window_of_job against a row-by-row statement, and mstep_span on random supports: n_lo <= n_hi or nothing to
//      stream, whole half-chunks, never beyond min(Np, n_ext), and the range covers [nlo, min(nhi, n_ext));
//   4. the first-maximum rule: a 64-row tile of random scores with planted exact ties and planted windows, replayed
//      through mstep_best_of_rows (lane), mstep_beats_tied (the 16 / 32 xor-shuffle merge, replayed here),
//      mstep_merge_waves and mstep_row_or_fallback, against "the first row of the maximum within [lo, hi) and < nrows",
//      the empty window included;
//   5. mstep_c0: the sentinel product rounded on its own, then one fused multiply-add - on a case where a product
//      rounded before the sum, and one where an unrounded sentinel product, give another f64.
#include "../scape_amd/csrc/scape_hip.hip"

#include <random>

static int g_fail = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            if (g_fail < 20) {                   \
                fprintf(stderr, "FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); \
                fprintf(stderr, __VA_ARGS__);    \
                fprintf(stderr, "\n");           \
            }                                    \
            ++g_fail;                            \
        }                                        \
    } while (0)

static void check_block() {
    long blocks = 0, live = 0;
    for (int n_utr = 1; n_utr <= 20; ++n_utr)
        for (int extent = 1; extent <= 5; ++extent) {
            const int grid = ((n_utr + 7) / 8) * 8 * extent;
            std::vector<int> seen((size_t)n_utr * extent, 0), residue(n_utr, -1);
            for (int id = 0; id < grid; ++id, ++blocks) {
                int ul = -1, t = -1;
                if (!mstep_block(id, n_utr, extent, ul, t)) {
                    CHECK(ul >= n_utr || t >= extent, "block %d of (%d, %d) rejected with (%d, %d)", id, n_utr, extent, ul, t);
                    continue;
                }
                CHECK(ul >= 0 && ul < n_utr && t >= 0 && t < extent, "block %d of (%d, %d) -> (%d, %d)", id, n_utr, extent, ul, t);
                if (ul < 0 || ul >= n_utr || t < 0 || t >= extent) continue;
                ++seen[(size_t)ul * extent + t];
                ++live;
                if (n_utr >= 8) {
                    CHECK(residue[ul] < 0 || residue[ul] == id % 8, "UTR %d of %d on XCDs %d and %d", ul, n_utr, residue[ul], id % 8);
                    residue[ul] = id % 8;
                }
            }
            for (size_t i = 0; i < seen.size(); ++i)
                CHECK(seen[i] == 1, "(%d UTRs, extent %d): pair %zu taken %d times", n_utr, extent, i, seen[i]);
        }
    printf("mstep_block: %ld blocks, %ld live pairs\n", blocks, live);
}

// Where each f64 of a slot came from (16 slot row + bin), the slot written as the DMA wavefronts write it: a piece is
// 1 KB, lane l of the instruction writes the 16 B at 16 l - the f64 pair that starts at bin m3_src_unit(slot row, l & 7).
static void write_piece(std::vector<int> &img, int byte0, int row_of_lane0, const char *what) {
    for (int l = 0; l < 64; ++l) {
        const int r = row_of_lane0 + (l >> 3), bin = m3_src_unit(r, l & 7);
        CHECK(bin >= 0 && bin + 1 < M3_CH && bin % 2 == 0, "%s %d lane %d fetches bin %d", what, r, l, bin);
        for (int e = 0; e < 2; ++e) {
            int &dst = img[(size_t)byte0 / 8 + 2 * l + e];
            CHECK(dst == -1, "%s %d lane %d overwrites", what, r, l);
            dst = 16 * r + bin + e;
        }
    }
}
// a tile slot (k3_mstep, k4_mstep): piece pc = tile rows 8 pc .. 8 pc + 7 at byte 1024 pc
static std::vector<int> tile_image() {
    std::vector<int> img(64 * M3_CH, -1);
    for (int pc = 0; pc < 8; ++pc) write_piece(img, 1024 * pc, 8 * pc, "tile row");
    return img;
}
// a job-vector slot of 4 column groups, by k4_mstep's roles: vector wavefront `role` (0 / 1) writes, for column group q,
// job slots js = 8 (2 q + role) .. + 7 at byte 2048 q + 1024 role; k3_mstep's piece i = job slots 8 i .. at byte 1024 i
// is the same place
static std::vector<int> vector_image() {
    std::vector<int> img(64 * M3_CH, -1);
    for (int q = 0; q < 4; ++q)
        for (int role = 0; role < 2; ++role) {
            const int i = 2 * q + role;
            CHECK(2048 * q + 1024 * role == 1024 * i, "the two kernels place job slots %d.. differently", 8 * i);
            write_piece(img, 2048 * q + 1024 * role, 8 * (2 * q + role), "job slot");
        }
    return img;
}
static void check_swizzle() {
    const std::vector<int> tile = tile_image(), vec = vector_image();
    long reads = 0, groups = 0;
    for (int pass = 0; pass < 2; ++pass)                        // 0: the A fragment of wavefront w, 1: the B fragment of column group w
        for (int w = 0; w < 4; ++w)
            for (int s = 0; s < 4; ++s)
                for (int half = 0; half < 2; ++half) {          // a ds_read_b64 is served 32 lanes at a time: 16 rows x 2 taps
                    unsigned banks = 0u;
                    for (int l = 32 * half; l < 32 * half + 32; ++l) {
                        const int kq = l >> 4, rc = l & 15, offd = m3_frag_index(s, kq, rc);
                        // m3_stream / m4_seg: ts = slot + (16 wave + rc) M3_CH, read ts[offd];
                        // mstep_kstep: vs = slot + rc M3_CH, read vs[g 16 M3_CH + offd]
                        const int idx = pass == 0 ? (16 * w + rc) * M3_CH + offd : rc * M3_CH + w * 16 * M3_CH + offd;
                        const std::vector<int> &img = pass == 0 ? tile : vec;
                        CHECK(idx >= 0 && idx < 64 * M3_CH, "index %d", idx);
                        CHECK(img[idx] == 16 * (16 * w + rc) + 4 * s + kq, "%s %d, bin %d: read (%d, %d)", pass ? "job slot" : "tile row",
                              16 * w + rc, 4 * s + kq, img[idx] / 16, img[idx] % 16);
                        banks |= 1u << (idx % 32);              // 64 banks of 4 B = 32 pairs
                        ++reads;
                    }
                    CHECK(banks == 0xffffffffu, "pass %d group %d, k-step %d, lanes %d..: bank pairs %08x", pass, w, s, 32 * half, banks);
                    ++groups;
                }
    printf("swizzle: %ld fragment reads in %ld 32-lane groups (tile slot and job-vector slot), 2 x 8 pieces x 64 lanes written\n", reads, groups);
}

// The constant part of a score: SENT * tl rounded on its own, then ONE fused multiply-add of lw * sv onto it.
static void check_c0() {
    // no tail: the rounded product alone
    CHECK(mstep_c0(3.0, 0.5, 0.0) == 1.5 && mstep_c0(-2.5, 4.0, 0.0) == -10.0, "mstep_c0 without a tail");
    // fused: with s = SENT 2^-10 (exact) and lw sv = -s (1 + 2^-40), the exact sum is -s 2^-40; a product rounded on its
    // own loses its low 11 bits first
    const double tl = 0x1p-10, s = SENT * tl, lw = -s, sv = 1.0 + 0x1p-40;
    volatile double prod = lw * sv;
    const double two_step = prod + s, exact = std::ldexp(lw, -40);
    CHECK(two_step != exact, "the case does not tell a fused from an unfused evaluation");
    CHECK(mstep_c0(lw, sv, tl) == exact, "mstep_c0 rounds lw * sv before the sum: %a, exact %a", mstep_c0(lw, sv, tl), exact);
    // the sentinel product is rounded to f64 before it enters: SENT (24 bits) x (1 + 2^-40) needs 64 bits - exact in the
    // 64-bit mantissa of long double, one rounding from there to f64
    const double tl2 = 1.0 + 0x1p-40;
    const long double wide = (long double)SENT * (long double)tl2;
    const double rounded = (double)wide;
    CHECK((long double)rounded != wide, "the case does not round");
    // ... so lw sv = -rounded cancels it exactly; an evaluation that kept the product's low bits would leave them
    CHECK(mstep_c0(0.0, 1.0, tl2) == rounded && mstep_c0(-rounded, 1.0, tl2) == 0.0, "mstep_c0's sentinel product: %a", mstep_c0(-rounded, 1.0, tl2));
    CHECK((double)(wide - (long double)rounded) != 0.0, "the case does not tell a separately rounded product");
    printf("mstep_c0: no tail, fused sum, separately rounded sentinel product\n");
}

static void check_window_and_span(std::mt19937_64 &rng, int n_cases) {
    for (int it = 0; it < n_cases; ++it) {
        // ---- one job's window against the tile, row by row
        const int t = (int)(rng() % 6), row0 = t * MT_ROWS;
        // (a window is never empty: rd_hi = (hi + 1) B > rd_lo = lo B)
        const int lo = (rng() % 4 == 0) ? row0 + (int)(rng() % MT_ROWS) : (int)(rng() % (8 * MT_ROWS));
        const int hi = (rng() % 4 == 0) ? std::max(lo + 1, row0 + (int)(rng() % (MT_ROWS + 2))) : lo + 1 + (int)(rng() % (3 * MT_ROWS));
        const int n0 = (int)(rng() % 300), n1 = (rng() % 8 == 0) ? n0 : n0 + (int)(rng() % 300);
        const MstepWin w = mstep_window_of_job(lo, hi, n0, n1, row0, t);
        int mk = 0;
        for (int r = row0; r < row0 + MT_ROWS; ++r)
            if (r >= lo && r < hi) mk |= 1 << ((r - row0) / 16);
        CHECK(w.mk == mk, "window [%d, %d) on tile %d: groups %x, by rows %x", lo, hi, t, w.mk, mk);
        CHECK(w.first == (lo >= row0 && lo < row0 + MT_ROWS), "window [%d, %d) on tile %d: first %d", lo, hi, t, w.first);
        CHECK(n1 > n0 ? (w.nlo == n0 && w.nhi == n1) : (w.nlo == 0x7fffffff && w.nhi == 0), "support [%d, %d) -> [%d, %d)", n0, n1, w.nlo, w.nhi);
        // ---- the streamed range of a pass
        const int Np = 16 * (1 + (int)(rng() % 40));
        const int n_ext = (rng() % 6 == 0) ? 0 : 16 * (int)(rng() % (Np / 16 + 1));
        int nlo = 0x7fffffff, nhi = 0;                          // the empty support
        if (rng() % 6) {
            nlo = (int)(rng() % Np);
            nhi = nlo + 1 + (int)(rng() % (Np - nlo));
        }
        const MstepSpan sp = mstep_span(nlo, nhi, Np, n_ext);
        CHECK(sp.nh >= 0 && (sp.n_lo <= sp.n_hi || sp.nh == 0), "span [%d, %d) nh %d", sp.n_lo, sp.n_hi, sp.nh);
        CHECK(sp.n_lo >= 0 && sp.n_lo % 16 == 0 && sp.n_hi % 16 == 0, "span [%d, %d) off the half-chunk grid", sp.n_lo, sp.n_hi);
        if (sp.n_hi > sp.n_lo) CHECK(sp.nh * 16 == sp.n_hi - sp.n_lo, "span [%d, %d) nh %d", sp.n_lo, sp.n_hi, sp.nh);
        else CHECK(sp.nh == 0, "span [%d, %d) nh %d", sp.n_lo, sp.n_hi, sp.nh);
        CHECK(sp.n_hi <= std::min(Np, n_ext), "span ends at %d, Np %d, extent %d", sp.n_hi, Np, n_ext);
        const int want_hi = std::min(nhi, n_ext);               // bins the stream has to deliver: [nlo, want_hi)
        if (nhi > 0 && want_hi > nlo)
            CHECK(sp.nh > 0 && sp.n_lo <= nlo && sp.n_hi >= want_hi, "support [%d, %d), extent %d: streamed [%d, %d)", nlo, nhi, n_ext, sp.n_lo, sp.n_hi);
        if (nhi == 0) CHECK(sp.nh == 0, "empty support streams %d half-chunks", sp.nh);
        CHECK(mstep_tail_index(16 * (int64_t)it, it, n_ext) == (int64_t)it + it + n_ext / 16, "tail index");
    }
    printf("window and span: %d random cases\n", n_cases);
}

static void check_first_maximum(std::mt19937_64 &rng, int n_cases) {
    long ties = 0, empty = 0;
    std::uniform_real_distribution<double> uni(-1e3, 1e3);
    for (int it = 0; it < n_cases; ++it) {
        const int t = (int)(rng() % 4), row0 = t * MT_ROWS;
        const int nrows = row0 + 1 + (int)(rng() % (2 * MT_ROWS));          // the tile may be the partial last one
        int lo = std::max(0, row0 - MT_ROWS / 2 + (int)(rng() % (3 * MT_ROWS / 2))), hi = lo + 1 + (int)(rng() % (2 * MT_ROWS));
        if (rng() % 8 == 0) hi = lo;                                        // planted: the empty window
        if (rng() % 8 == 0) lo = hi = nrows + (int)(rng() % 5);             // ... and one beyond the tensor
        const double c0 = uni(rng);
        double acc[MT_ROWS];
        for (double &a : acc) a = uni(rng);
        const int n_tied = (int)(rng() % 6);                                // planted: exact ties, often of the maximum
        const double top = (rng() % 2) ? 2e3 : uni(rng);
        for (int q = 0; q < n_tied; ++q) acc[rng() % MT_ROWS] = top;
        // ---- plain statement
        int want = -1;
        for (int r = row0; r < row0 + MT_ROWS; ++r)
            if (r >= lo && r < hi && r < nrows && (want < 0 || c0 + acc[r - row0] > c0 + acc[want - row0])) want = r;
        int n_top = 0;
        for (int r = row0; want >= 0 && r < row0 + MT_ROWS; ++r)
            n_top += r >= lo && r < hi && r < nrows && c0 + acc[r - row0] == c0 + acc[want - row0];
        ties += n_top > 1;
        empty += want < 0;
        // ---- the kernels' path: D lane (kq, col) register i = row kq + 4 i of the wavefront's 16
        double ps[4];
        int pr[4];
        for (int wave = 0; wave < 4; ++wave) {
            MstepBest lane[4];
            for (int kq = 0; kq < 4; ++kq) {
                v4f64 frag;
                for (int i = 0; i < 4; ++i) frag[i] = acc[16 * wave + kq + 4 * i];
                lane[kq] = mstep_best_of_rows(MstepBest{}, frag, c0, lo, hi, row0 + 16 * wave + kq, nrows);
            }
            for (int off = 1; off <= 2; off <<= 1) {                        // lanes 16 and 32 apart: kq ^ 1, kq ^ 2
                MstepBest next[4];
                for (int kq = 0; kq < 4; ++kq) {
                    const MstepBest &o = lane[kq ^ off];
                    next[kq] = mstep_beats_tied(o.score, o.row, lane[kq]) ? o : lane[kq];
                }
                for (int kq = 0; kq < 4; ++kq) lane[kq] = next[kq];
            }
            for (int kq = 1; kq < 4; ++kq)
                CHECK(lane[kq].row == lane[0].row && lane[kq].score == lane[0].score, "the four lanes of wavefront %d disagree", wave);
            ps[wave] = lane[0].score;
            pr[wave] = lane[0].row;
        }
        const MstepBest b = mstep_merge_waves(ps, pr, 1, 0);
        const int got = mstep_row_or_fallback(b.row, lo, row0);
        if (want >= 0) {
            CHECK(got == want && b.score == c0 + acc[want - row0], "window [%d, %d), tile %d, %d rows: row %d, want %d", lo, hi, t, nrows, got, want);
        } else {
            CHECK(b.row == 0x7fffffff && b.score == -INFINITY && got == std::max(lo, row0), "empty window [%d, %d) on tile %d: row %d", lo, hi, t, got);
        }
    }
    printf("first maximum: %d tiles, %ld with a tied maximum, %ld with an empty window\n", n_cases, ties, empty);
    CHECK(ties > n_cases / 20 && empty > n_cases / 20, "the planted cases did not come up");
}

int main() {
    std::mt19937_64 rng(20261021);
    check_block();
    check_swizzle();
    check_window_and_span(rng, 200000);
    check_first_maximum(rng, 200000);
    check_c0();
    if (g_fail) {
        fprintf(stderr, "%d checks FAILED\n", g_fail);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
