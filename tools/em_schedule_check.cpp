// em_schedule_check.cpp - host check of the EM run-ahead schedule and of em_plan's column tables (no GPU needed).
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined \
//         -o em_schedule_check tools/em_schedule_check.cpp && ./em_schedule_check
// (main makes no HIP call; the sanitizers instrument the host side only)
//
// The program includes the library's source, so it drives the very em_run_ahead_stops (the rule k2_estep
// applies, em_lockstep.inc) and em_plan (scape_hip.hip) the library is built from, and compares them with plain
// restatements written here:
//   1. random component orders (K = 1..12, 1..50 rounds, depth 1..4, a random stopping round): the passes the rule cuts a
//      job's rounds into are replayed; no pass may hold two columns whose components are equal or adjacent, none a round
//      whose own component or index neighbour has its arg-max pending, every pass runs 1..depth consecutive rounds, and
//      depth 1 is one round per pass;
//   2. random calls: em_plan's ujoff / ujlist / voff / ptoff / elist / totals for depth 1..4 against a direct count.
#include "../scape_amd/csrc/scape_hip.hip"

#include <random>
#include <set>

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

struct Pass {
    std::vector<int> rounds;
};

// the slots of a pass (k2_estep, em_rounds) for one non-fixed job that stops after round `last` (stopping rule) or at the cap
static std::vector<Pass> run_rule(const std::vector<int> &k_arr, int K, int depth, int last) {
    const int nround = (int)k_arr.size();
    std::vector<Pass> passes;
    int nlb = 0, status = 0;
    while (status == 0 && nlb < nround) {
        Pass p;
        unsigned long long pend = 0ull;
        for (int slot = 0; slot < depth; ++slot) {
            const int k = k_arr[nlb];
            p.rounds.push_back(nlb);
            status = (nlb == last) ? 1 : 0;
            ++nlb;
            if (k < K) pend |= 2ull << k;          // the round published a column (estep_body: has_m)
            const int k_next = k_arr[std::min(nlb, nround - 1)];
            if (em_run_ahead_stops(status, nlb, nround, k_next, pend)) break;
        }
        passes.push_back(p);
    }
    return passes;
}

static long check_schedules(std::mt19937_64 &rng, int n_cases) {
    long job_rounds = 0, job_passes = 0;
    for (int it = 0; it < n_cases; ++it) {
        const int K = 1 + (int)(rng() % 12), nround = 1 + (int)(rng() % 50), depth = 1 + (int)(rng() % 4);
        // gen_k_arr: permutations of the K components, the uniform component K mixed in now and then (any order must do)
        std::vector<int> k_arr(nround), perm(K);
        for (int i = 0; i < K; ++i) perm[i] = i;
        for (int t0 = 0; t0 < nround; t0 += K) {
            std::shuffle(perm.begin(), perm.end(), rng);
            for (int i = 0; i < K && t0 + i < nround; ++i) k_arr[t0 + i] = (rng() % 16 == 0) ? K : perm[i];
        }
        if (rng() % 8 == 0)
            for (int &k : k_arr) k = (int)(rng() % (K + 1));     // no structure at all
        const int last = (rng() % 3 == 0) ? nround - 1 : (int)(rng() % nround);
        const std::vector<Pass> passes = run_rule(k_arr, K, depth, last);
        int next = 0;
        for (const Pass &p : passes) {
            CHECK(!p.rounds.empty() && (int)p.rounds.size() <= depth, "pass of %zu rounds at depth %d", p.rounds.size(), depth);
            if (depth == 1) CHECK(p.rounds.size() == 1, "depth 1 must be one round per pass");
            std::set<int> pending;                     // components published earlier in this pass: arg-max not yet taken
            for (int r : p.rounds) {
                CHECK(r == next, "round %d where %d was due", r, next);
                ++next;
                const int c = k_arr[r];
                CHECK(!pending.count(c - 1) && !pending.count(c) && !pending.count(c + 1),
                      "K %d depth %d round %d: component %d runs with a pending neighbour", K, depth, r, c);
                if (c < K) {
                    for (int o : pending) CHECK(std::abs(o - c) > 1, "columns of components %d and %d share a pass", o, c);
                    pending.insert(c);
                }
            }
        }
        CHECK(next == last + 1, "the job ran %d rounds, stops after round %d", next, last);
        CHECK((int)passes.size() <= next, "more passes than rounds");
        job_rounds += next;
        job_passes += (long)passes.size();
    }
    printf("schedule: %d jobs, %ld job-rounds in %ld job-passes\n", n_cases, job_rounds, job_passes);
    return job_rounds;
}

static void check_plans(std::mt19937_64 &rng, int n_cases) {
    for (int it = 0; it < n_cases; ++it) {
        const int n_utr = 1 + (int)(rng() % 40), B = 1 + (int)(rng() % 13), depth = 1 + (int)(rng() % 4);
        const size_t nj = 1 + (size_t)(rng() % 300);
        const bool size_order = rng() % 2;
        std::vector<UtrDesc> desc(n_utr);
        for (UtrDesc &d : desc) {
            memset(&d, 0, sizeof(d));
            d.T = 1 + (int)(rng() % 400);
            d.N = 1 + (int)(rng() % 2000);
            d.Np = (d.N + 15) / 16 * 16;
        }
        std::vector<int32_t> job_utr(nj), job_fixed(nj);
        const int mode = (int)(rng() % 3);
        for (size_t j = 0; j < nj; ++j) {
            job_utr[j] = (int32_t)(rng() % n_utr);
            job_fixed[j] = mode == 0 ? 1 : mode == 1 ? 0 : (int32_t)(rng() % 2);
        }
        if (rng() % 2) std::sort(job_utr.begin(), job_utr.end());
        const EmPlan p = em_plan(desc, B, nj, job_utr.data(), job_fixed.data(), size_order, depth);
        // restatement
        CHECK(p.depth == depth, "depth");
        CHECK(p.voff.size() == nj * depth && p.ptoff.size() == nj * depth && p.ujlist.size() == nj * depth, "table sizes");
        size_t v = 0, pt = 0;
        bool any_m = false;
        for (size_t j = 0; j < nj; ++j) {
            const UtrDesc &d = desc[job_utr[j]];
            const size_t tiles = (size_t)((d.T * B + MT_ROWS - 1) / MT_ROWS);
            for (int q = 0; q < depth; ++q) {
                CHECK(p.voff[j * depth + q] == (int64_t)v && p.ptoff[j * depth + q] == (int64_t)pt, "offsets of job %zu slot %d", j, q);
                CHECK(v % 16 == 0, "job vectors start on 128-byte lines");
                v += (size_t)d.Np;
                pt += tiles;
            }
            any_m = any_m || !job_fixed[j];
        }
        CHECK(p.vtot == v && p.pttot == pt && p.any_m == any_m, "totals");
        int max_cols = 1, tiles_max = 1;
        std::vector<int32_t> active;
        for (int u = 0; u < n_utr; ++u) {
            std::vector<int32_t> cols;
            for (size_t j = 0; j < nj; ++j)
                if (job_utr[j] == u)
                    for (int q = 0; q < depth; ++q) cols.push_back((int32_t)(j * depth + q));
            CHECK(p.ujoff[u + 1] - p.ujoff[u] == (int64_t)cols.size(), "columns of UTR %d", u);
            for (size_t i = 0; i < cols.size(); ++i) CHECK(p.ujlist[p.ujoff[u] + i] == cols[i], "column list of UTR %d", u);
            if (!cols.empty()) {
                active.push_back(u);
                max_cols = std::max(max_cols, (int)cols.size());
                tiles_max = std::max(tiles_max, (desc[u].T * B + MT_ROWS - 1) / MT_ROWS);
            }
        }
        CHECK(p.max_cols_utr == max_cols && p.tiles_max == tiles_max, "maxima");
        std::vector<int32_t> act = p.active;
        std::sort(act.begin(), act.end());
        CHECK(act == active, "active UTRs");
        if (size_order)
            for (size_t i = 1; i < p.active.size(); ++i)
                CHECK((int64_t)desc[p.active[i - 1]].T * desc[p.active[i - 1]].Np >= (int64_t)desc[p.active[i]].T * desc[p.active[i]].Np,
                      "size order");
        // the E-step list: every job once, the jobs of a UTR together and in job order
        CHECK(p.elist.size() == nj, "E-step list size");
        std::vector<int> seen(nj, 0);
        for (size_t i = 0; i < p.elist.size(); ++i) {
            const int32_t j = p.elist[i];
            CHECK(j >= 0 && (size_t)j < nj && !seen[j], "E-step list entry %zu", i);
            if (j >= 0 && (size_t)j < nj) seen[j] = 1;
            if (i && job_utr[p.elist[i - 1]] == job_utr[j]) CHECK(p.elist[i - 1] < j, "job order inside a UTR");
        }
        std::set<int> closed;
        for (size_t i = 0; i < p.elist.size(); ++i) {
            const int u = job_utr[p.elist[i]];
            if (i && job_utr[p.elist[i - 1]] != u) closed.insert(job_utr[p.elist[i - 1]]);
            CHECK(!closed.count(u), "the jobs of UTR %d are not contiguous in the E-step list", u);
        }
    }
    printf("em_plan: %d random calls\n", n_cases);
}

int main() {
    std::mt19937_64 rng(20261018);
    check_schedules(rng, 200000);
    check_plans(rng, 3000);
    if (g_fail) {
        fprintf(stderr, "%d checks FAILED\n", g_fail);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
