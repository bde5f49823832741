// batch_plan_check.cpp - host check of batch_plan (the descriptor walk of scape_hip_batch_load) and of the Phase B choice
// of scape_hip_batch_build (no GPU needed).
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined \
//         -o batch_plan_check tools/batch_plan_check.cpp && ./batch_plan_check
// (main makes no HIP call; the sanitizers instrument the host side only)
//
// The program includes the library's source, so it drives the very batch_plan and phase_b_choose the library is built
// from, and compares them with plain restatements written here:
//   1. random batches (1-12 UTRs of 1-200 bins and 1-120 grid points, every grid kind, n_beta 1-20);
//   2. batches on both sides of every boundary the walk has: N at multiples of PITCH and +-1, T * n_beta at multiples
//      of TILE_ROWS and +-1, n_log at 0 / PB_LOGCAP / PB_LOGCAP + 1, uniform integer grids with and without interior
//      points, a non-integer and a non-uniform grid, n_beta 16 and 17, W_max at 4 * PB_STEPS and one more, T_max at
//      4096 and 4097;
//   3. every refusal of the walk, with the arrays the refused UTR would index left out: a walk that read them before it
//      refused would run into the sanitizer;
//   4. phase_b_choose over a grid of n_beta x window x T_max x slide x SCAPE_HIP_PHASE_B, refusals included.
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

enum Grid { UNIFORM, UNIFORM_HALF, NON_UNIFORM, REPEATS };   // integer steps; steps of 0.5 from 0.5; uneven steps; ties

struct Utr {
    int N, T, n_log;       // bins, grid points, bins that are not all-NaN in (pa, r)
    Grid grid;
    double step;
};

struct Batch {
    scape_hip_params p;
    std::vector<int64_t> bin_off, theta_off;
    std::vector<double> theta, r, pa, L, min_theta, unif_ll;
};

static Batch make_batch(std::mt19937_64 &rng, int n_beta, double bmax, const std::vector<Utr> &utrs) {
    Batch b;
    memset(&b.p, 0, sizeof(b.p));
    b.p.n_beta = n_beta;
    b.p.n_s = 1;
    b.p.nround = 50;
    for (int j = 0; j < n_beta; ++j) b.p.betas[j] = bmax * (j + 1) / n_beta;
    std::swap(b.p.betas[0], b.p.betas[rng() % n_beta]);       // the widest beta stands anywhere
    b.bin_off.push_back(0);
    b.theta_off.push_back(0);
    const double nan = std::nan("");
    for (const Utr &u : utrs) {
        b.bin_off.push_back(b.bin_off.back() + u.N);
        b.theta_off.push_back(b.theta_off.back() + u.T);
        double t = u.grid == UNIFORM_HALF ? 0.5 : (double)(rng() % 500);
        for (int i = 0; i < u.T; ++i) {
            b.theta.push_back(t);
            if (u.grid == NON_UNIFORM) t += u.step * (1 + (i % 3 == 1));
            else if (u.grid == REPEATS) t += (i % 2) ? u.step : 0.0;
            else t += u.step;
        }
        std::vector<char> is_log(u.N, 0);
        for (int k = 0; k < u.n_log; ++k) is_log[k] = 1;
        std::shuffle(is_log.begin(), is_log.end(), rng);
        for (int n = 0; n < u.N; ++n) {
            const int kind = is_log[n] ? 1 + (int)(rng() % 3) : 0;      // pa known, r known, both
            b.pa.push_back(kind & 1 ? 20.0 : nan);
            b.r.push_back(kind & 2 ? 300.0 : nan);
        }
        b.L.push_back(1000.0 + (double)(rng() % 1000));
        b.min_theta.push_back((double)(rng() % 50));
        b.unif_ll.push_back(-std::log(b.L.back()));
    }
    return b;
}

static int plan_of(const Batch &b, BatchPlan &plan) {
    return batch_plan(b.p, (int)b.bin_off.size() - 1, b.bin_off.data(), b.theta_off.data(), b.theta.data(), b.r.data(),
                      b.pa.data(), b.L.data(), b.min_theta.data(), b.unif_ll.data(), plan);
}

// the restatement: every figure from its definition, offsets as sums over the UTRs ahead
static void check_batch(const Batch &b, const char *what) {
    BatchPlan plan;
    CHECK(plan_of(b, plan) == 0, "%s: refused: %s", what, g_err.c_str());
    const int n_utr = (int)b.bin_off.size() - 1, B = b.p.n_beta;
    const double bmax = *std::max_element(b.p.betas, b.p.betas + B);
    CHECK(plan.n_utr == n_utr && (int)plan.h_desc.size() == n_utr, "%s: n_utr", what);
    if ((int)plan.h_desc.size() != n_utr) return;
    int64_t at = 0, m = 0, tiles = 0, mlog = 0;
    int T_max = 0, Np_max = 0, W_max = 1, tiles_max = 1;
    bool slide = B <= 16;
    std::vector<int32_t> loglist, logbin;
    for (int u = 0; u < n_utr; ++u) {
        const UtrDesc &d = plan.h_desc[u];
        const int64_t N = b.bin_off[u + 1] - b.bin_off[u], T = b.theta_off[u + 1] - b.theta_off[u];
        const double *th = b.theta.data() + b.theta_off[u];
        const int64_t Np = (N + PITCH - 1) / PITCH * PITCH, nt = (T * B + TILE_ROWS - 1) / TILE_ROWS;
        CHECK(d.bin_off == b.bin_off[u] && d.theta_off == b.theta_off[u] && d.N == N && d.T == T && d.Np == Np,
              "%s: UTR %d sizes", what, u);
        CHECK(d.at_off == at && d.m_off == m && d.tile_off == tiles && d.mlog_off == mlog && d.log_off == (int64_t)loglist.size(),
              "%s: UTR %d offsets", what, u);
        CHECK(d.unif_ll == b.unif_ll[u] && d.L == b.L[u] && d.min_theta == b.min_theta[u], "%s: UTR %d constants", what, u);
        int n_log = 0;
        for (int64_t n = 0; n < N; ++n)
            if (!(std::isnan(b.pa[b.bin_off[u] + n]) && std::isnan(b.r[b.bin_off[u] + n]))) {
                loglist.push_back((int32_t)n);
                logbin.push_back(u);
                ++n_log;
            }
        CHECK(d.n_log == n_log, "%s: UTR %d n_log %d, want %d", what, u, d.n_log, n_log);
        // uniform: at least two points, all integers, one positive step
        bool uni = T > 1 && th[1] > th[0];
        for (int64_t i = 0; i < T; ++i) uni = uni && th[i] == std::rint(th[i]) && (i == 0 || th[i] - th[i - 1] == th[1] - th[0]);
        int c_lo = 1, c_hi = 0;
        if (uni) {
            const int reach = (int)std::floor(3 * bmax / (th[1] - th[0])) + 1;
            c_lo = reach + 1;
            c_hi = (int)T - 2 - reach;
        }
        CHECK(d.c_lo == c_lo && d.c_hi == c_hi, "%s: UTR %d interior [%d, %d], want [%d, %d]", what, u, d.c_lo, d.c_hi, c_lo, c_hi);
        slide = slide && c_lo <= c_hi;
        // the widest window: grid points within 3 * bmax of a grid point, ends included
        for (int64_t i = 0; i < T; ++i)
            W_max = std::max(W_max, (int)(std::upper_bound(th, th + T, th[i] + 3 * bmax) - std::lower_bound(th, th + T, th[i] - 3 * bmax)));
        at += T * Np;
        m += T * B * Np;
        tiles += nt;
        if (n_log >= 1 && n_log <= PB_LOGCAP) mlog += T * B * n_log;
        T_max = std::max(T_max, (int)T);
        Np_max = std::max(Np_max, (int)Np);
        tiles_max = std::max(tiles_max, (int)nt);
    }
    slide = slide && W_max <= 4 * PB_STEPS && T_max <= 4096;
    CHECK(plan.loglist == loglist && plan.logbin_utr == logbin && plan.n_logbins == logbin.size(), "%s: log-domain bin lists", what);
    CHECK((int64_t)plan.at_total == at && (int64_t)plan.m_total == m && (int64_t)plan.tiles_total == tiles &&
              (int64_t)plan.mlog_total == mlog, "%s: totals", what);
    CHECK(plan.n_bins == b.bin_off[n_utr] && (int64_t)plan.n_theta_total == b.theta_off[n_utr], "%s: array lengths", what);
    CHECK(plan.T_max == T_max && plan.Np_max == Np_max && plan.tiles_max_all == tiles_max, "%s: maxima", what);
    CHECK(plan.W_max == W_max, "%s: W_max %d, want %d", what, plan.W_max, W_max);
    CHECK(plan.pb_slide == slide, "%s: pb_slide %d, want %d", what, (int)plan.pb_slide, (int)slide);
}

static void check_refused(const Batch &b, const char *message, const char *what) {
    BatchPlan plan;
    plan.n_utr = -7;
    CHECK(plan_of(b, plan) == 1 && g_err.find(message) != std::string::npos, "%s: not refused with '%s' (%s)", what, message, g_err.c_str());
    CHECK(plan.n_utr == -7 && plan.h_desc.empty(), "%s: a refused walk wrote its result", what);
}

// the Phase B choice from its rule, the LDS sizes in bytes from the kernels' layouts (phase_b.inc)
static void check_choice(int B, int W, int T_max, bool slide, const char *mode) {
    PhaseB ch;
    const int rc = phase_b_choose(B, W, T_max, slide, mode, ch);
    const std::string m = mode ? mode : "";
    const int form = (B > 16 || m == "v2") ? 0 : m == "split" ? 1 : slide ? 2 : 0;
    const size_t WP = (size_t)(W + 3) / 4 * 4 + 1;
    CHECK(ch.form == form && ch.Wmax == W && (size_t)ch.WP == WP, "choice B %d W %d mode %s: form %d, want %d", B, W, m.c_str(), ch.form, form);
    if (form == 0) {
        const size_t lds = 8 * ((size_t)2 * B * W + B) + 4 * (size_t)2 * (B + 1) + 8 * 16 * WP;
        CHECK(ch.lds == lds && rc == (lds > 150 * 1024), "choice B %d W %d: form 0 LDS %zu, want %zu, rc %d", B, W, ch.lds, lds, rc);
    } else {
        const size_t lds_t = 8 * ((size_t)B * W + 16) + 4 * 32, lds_l = 8 * (16 * WP + 16 * PB_LOGCAP) + 4 * PB_LOGCAP;
        const size_t lds_c = 8 * ((size_t)(T_max + T_max % 2) + (size_t)B * W) + 4 * 16, lds_s = 8 * (16 * WP + 4 * PB_RING * 16);
        CHECK(ch.lds_t == lds_t && ch.lds_l == lds_l && ch.lds_c == lds_c && ch.lds_s == lds_s, "choice B %d W %d: LDS sizes", B, W);
        CHECK(rc == (lds_t > 60 * 1024 || lds_l > 60 * 1024), "choice B %d W %d: rc %d", B, W, rc);
    }
    if (rc) CHECK(g_err.find("does not fit LDS") != std::string::npos, "refusal message: %s", g_err.c_str());
}

int main() {
    std::mt19937_64 rng(20261019);
    long n_batches = 0;
    // 1. random batches
    for (int it = 0; it < 4000; ++it) {
        const int n_beta = 1 + (int)(rng() % 20);
        const double bmax = 1.0 + (double)(rng() % 40);
        std::vector<Utr> utrs(1 + rng() % 12);
        for (Utr &u : utrs) {
            u.N = 1 + (int)(rng() % 200);
            u.T = 1 + (int)(rng() % 120);
            u.n_log = (rng() % 3 == 0) ? 0 : (int)(rng() % (u.N + 1));
            u.grid = (rng() % 4 == 0) ? (Grid)(1 + rng() % 3) : UNIFORM;
            u.step = (u.grid == UNIFORM_HALF) ? 0.5 : (double)(1 + rng() % 12);
        }
        check_batch(make_batch(rng, n_beta, bmax, utrs), "random");
        ++n_batches;
    }
    // 2. the boundaries.  One UTR each unless said, n_beta = 4, widest beta 5 (reach 15 points at step 1) unless said.
    auto one = [&](int n_beta, double bmax, Utr u, const char *what) {
        check_batch(make_batch(rng, n_beta, bmax, {u}), what);
        check_batch(make_batch(rng, n_beta, bmax, {{33, 40, 5, UNIFORM, 1.0}, u, {7, 3, 0, UNIFORM, 2.0}}), what);   // and between two others
        n_batches += 2;
    };
    for (int k = 1; k <= 4; ++k)
        for (int dN = -1; dN <= 1; ++dN) one(4, 5.0, {k * PITCH + dN, 50, 3, UNIFORM, 1.0}, "N at a multiple of PITCH");
    for (int n_beta : {1, 4, 13, 16, 17})
        for (int rows = TILE_ROWS; rows <= 3 * TILE_ROWS; rows += TILE_ROWS)
            for (int dT = -1; dT <= 1; ++dT) {
                const int T = (rows + n_beta - 1) / n_beta + dT;      // T * n_beta on both sides of `rows`
                if (T >= 1) one(n_beta, 5.0, {20, T, 2, UNIFORM, 1.0}, "T * n_beta at a multiple of TILE_ROWS");
            }
    for (int T : {16, 32, 48, 64})                                     // exact multiples at n_beta 4: 64, 128, 192, 256 rows
        for (int dT = -1; dT <= 1; ++dT) one(4, 5.0, {20, T + dT, 2, UNIFORM, 1.0}, "T * 4 at a multiple of TILE_ROWS");
    for (int n_log : {0, 1, PB_LOGCAP - 1, PB_LOGCAP, PB_LOGCAP + 1, 200}) one(4, 5.0, {200, 50, n_log, UNIFORM, 1.0}, "n_log at PB_LOGCAP");
    // interior points: reach = floor(3 * 5 / step) + 1, c_lo = reach + 1, c_hi = T - 2 - reach: the first T with c_lo <= c_hi is 2 * reach + 3
    for (double step : {1.0, 2.0, 5.0, 15.0, 16.0})
        for (int dT = -1; dT <= 1; ++dT) {
            const int reach = (int)(15.0 / step) + 1;
            one(4, 5.0, {20, 2 * reach + 3 + dT, 2, UNIFORM, step}, "uniform grid with / without interior points");
        }
    for (int T : {1, 2, 3}) one(4, 5.0, {20, T, 2, UNIFORM, 1.0}, "shortest grids");
    one(4, 5.0, {20, 80, 2, UNIFORM_HALF, 0.5}, "non-integer grid");
    one(4, 5.0, {20, 80, 2, NON_UNIFORM, 1.0}, "non-uniform grid");
    one(4, 5.0, {20, 80, 2, REPEATS, 1.0}, "grid with repeated points");
    for (int n_beta : {16, 17}) one(n_beta, 5.0, {20, 80, 2, UNIFORM, 1.0}, "n_beta 16 / 17");
    // The window of a uniform grid is symmetric, so W_max is odd there: 2 * floor(3 * bmax) + 1 at step 1, 47 at
    // 3 * bmax = 23.5 and 49 at 24, which bracket 4 * PB_STEPS = 48 for pb_slide.  48 itself takes a grid with ties: 48
    // points in pairs 0, 0, 1, 1, ... 23, 23, all within 24 of each other, and the rest far apart.
    for (double bmax : {23.5 / 3, 8.0, 24.5 / 3}) one(4, bmax, {20, 200, 2, UNIFORM, 1.0}, "W_max at 4 * PB_STEPS");
    {
        BatchPlan plan;
        Batch b47 = make_batch(rng, 4, 23.5 / 3, {{20, 200, 2, UNIFORM, 1.0}}), b49 = make_batch(rng, 4, 8.0, {{20, 200, 2, UNIFORM, 1.0}});
        CHECK(plan_of(b47, plan) == 0 && plan.W_max == 47 && plan.pb_slide, "W_max 47 slides");
        CHECK(plan_of(b49, plan) == 0 && plan.W_max == 49 && !plan.pb_slide, "W_max 49 does not slide");
        Batch b48 = make_batch(rng, 4, 8.0, {{20, 200, 2, UNIFORM, 1.0}});
        for (size_t i = 0; i < b48.theta.size(); ++i) b48.theta[i] = (i < 48) ? (double)(i / 2) : 1000.0 + 100.0 * (double)i;
        check_batch(b48, "one window of 48");
        CHECK(plan_of(b48, plan) == 0 && plan.W_max == 48, "W_max %d, want 48", plan.W_max);
        ++n_batches;
    }
    for (int T : {4095, 4096, 4097}) one(4, 5.0, {20, T, 2, UNIFORM, 1.0}, "T_max at 4096");
    {
        BatchPlan plan;
        Batch b = make_batch(rng, 4, 5.0, {{20, 4096, 2, UNIFORM, 1.0}});
        CHECK(plan_of(b, plan) == 0 && plan.pb_slide, "T_max 4096 slides");
        b = make_batch(rng, 4, 5.0, {{20, 4097, 2, UNIFORM, 1.0}});
        CHECK(plan_of(b, plan) == 0 && !plan.pb_slide, "T_max 4097 does not slide");
    }
    // 3. refusals.  The refused UTR is the last one and its bins / grid points are not in the arrays.
    {
        const std::vector<Utr> good = {{33, 40, 5, UNIFORM, 1.0}, {20, 30, 0, UNIFORM, 2.0}};
        auto with_last = [&](int64_t N, int64_t T) {
            Batch b = make_batch(rng, 4, 5.0, good);
            b.bin_off.push_back(b.bin_off.back() + N);
            b.theta_off.push_back(b.theta_off.back() + T);
            b.L.push_back(1.0), b.min_theta.push_back(0.0), b.unif_ll.push_back(0.0);
            return b;
        };
        check_refused(with_last(0, 10), "UTR 2: bad n_frag / n_theta", "N = 0");
        check_refused(with_last(-1, 10), "UTR 2: bad n_frag / n_theta", "N < 0");
        check_refused(with_last(((int64_t)1 << 26) + 1, 10), "UTR 2: bad n_frag / n_theta", "N above 2^26");
        check_refused(with_last(10, 0), "UTR 2: bad n_frag / n_theta", "T = 0");
        check_refused(with_last(10, 65536), "UTR 2: bad n_frag / n_theta", "T above 65535");
        Batch b = make_batch(rng, 4, 5.0, good);
        std::swap(b.theta[45], b.theta[46]);
        check_refused(b, "UTR 1: all_theta must be ascending", "descending theta");
        b = make_batch(rng, 4, 5.0, good);
        b.theta[10] = std::nan("");
        check_refused(b, "UTR 0: all_theta must be ascending", "NaN in theta");
        check_batch(make_batch(rng, 4, 5.0, {{1, 65535, 1, UNIFORM, 1.0}}), "T = 65535");
    }
    // 4. the Phase B choice
    long n_choices = 0;
    for (int B : {1, 4, 13, 16, 17, 64, 160})
        for (int W : {1, 2, 3, 4, 5, 47, 48, 49, 60, 413, 414, 415, 477, 478, 479, 600})
            for (int T_max : {1, 2, 4095, 4096, 65535})
                for (int slide = 0; slide < 2; ++slide)
                    for (const char *mode : {(const char *)nullptr, "v2", "split", "slide", ""}) {
                        check_choice(B, W, T_max, slide != 0, mode);
                        ++n_choices;
                    }
    // ... and on the plans of loaded batches, as scape_hip_batch_build makes it
    for (int n_beta : {4, 16, 17})
        for (Grid g : {UNIFORM, NON_UNIFORM}) {
            BatchPlan plan;
            CHECK(plan_of(make_batch(rng, n_beta, 5.0, {{40, 80, 3, g, 1.0}}), plan) == 0, "plan");
            for (const char *mode : {(const char *)nullptr, "v2", "split"}) check_choice(n_beta, plan.W_max, plan.T_max, plan.pb_slide, mode);
        }
    printf("batch_plan: %ld batches; phase_b_choose: %ld choices\n", n_batches, n_choices);
    if (g_fail) {
        fprintf(stderr, "%d checks FAILED\n", g_fail);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
