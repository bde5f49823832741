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
//   3. the host halves of the shrink (em_rounds): em_slots_needed against the longest pass the rule gives any component
//      order over 0 .. K - 1, em_tiles_max on random live UTR lists, em_shrink_due at its edges, and k_em_shrink's in-place
//      chunked compaction (em_shrink_pos, replayed here thread by thread) against std::copy_if on random status vectors.
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

static void check_shrink(std::mt19937_64 &rng, int n_cases) {
    // slots: no pass of a job with K components uses more slots than em_slots_needed says, and the rule is what it claims
    for (int it = 0; it < n_cases * 20; ++it) {
        const int K = 1 + (int)(rng() % 12), nround = 1 + (int)(rng() % 50), depth = 1 + (int)(rng() % 4);
        std::vector<int> k_arr(nround), perm(K);
        for (int i = 0; i < K; ++i) perm[i] = i;
        for (int t0 = 0; t0 < nround; t0 += K) {
            std::shuffle(perm.begin(), perm.end(), rng);
            for (int i = 0; i < K && t0 + i < nround; ++i) k_arr[t0 + i] = perm[i];
        }
        if (rng() % 4 == 0)
            for (int &k : k_arr) k = (int)(rng() % K);           // any order over the K components
        const int slots = em_slots_needed(K, depth);
        CHECK(slots == std::min(depth, K <= 2 ? 1 : K == 3 ? 2 : depth), "slots rule, K %d depth %d", K, depth);
        for (const Pass &p : run_rule(k_arr, K, depth, nround - 1))
            CHECK((int)p.rounds.size() <= slots, "K %d depth %d: a pass of %zu rounds, %d slots launched", K, depth, p.rounds.size(), slots);
    }
    CHECK(em_slots_needed(0, 3) == 1 && em_slots_needed(3, 1) == 1 && em_slots_needed(63, 3) == 3, "slots rule at its ends");
    CHECK(!em_shrink_due(100, 100, 100) && em_shrink_due(100, 99, 100) && !em_shrink_due(100, 51, 50) && em_shrink_due(100, 50, 50) &&
              !em_shrink_due(100, 0, 100) && em_shrink_due(3, 1, 50) && !em_shrink_due(3, 2, 50),
          "em_shrink_due");
    for (int it = 0; it < n_cases; ++it) {
        // the M-step grid's second factor from a live UTR list
        const int n_utr = 1 + (int)(rng() % 40), B = 1 + (int)(rng() % 13);
        std::vector<UtrDesc> desc(n_utr);
        for (UtrDesc &d : desc) {
            memset(&d, 0, sizeof(d));
            d.T = 1 + (int)(rng() % 400);
        }
        std::vector<int32_t> live;
        for (int u = 0; u < n_utr; ++u)
            if (rng() % 3 == 0) live.push_back(u);
        std::shuffle(live.begin(), live.end(), rng);
        int want = 1;
        for (int32_t u : live) want = std::max(want, (desc[u].T * B + MT_ROWS - 1) / MT_ROWS);
        CHECK(em_tiles_max(desc, B, live.data(), (int)live.size()) == want, "tiles_max of %zu live UTRs", live.size());
        // the compaction: EM_SHRINK_THREADS entries per chunk, one per thread, in place
        const int n = 1 + (int)(rng() % 5000), mode = (int)(rng() % 4);
        std::vector<int32_t> list(n), status(n);
        for (int i = 0; i < n; ++i) list[i] = i;
        std::shuffle(list.begin(), list.end(), rng);
        for (int32_t &st : status) st = mode == 0 ? 2 : mode == 1 ? (int32_t)(rng() % 2) : (int32_t)(rng() % 3);
        if (mode == 3) std::fill(status.begin(), status.begin() + n / 2, 2);
        std::vector<int32_t> expect;
        std::copy_if(list.begin(), list.end(), std::back_inserter(expect), [&](int32_t j) { return status[j] != 2; });
        constexpr int NW = EM_SHRINK_THREADS / 64;
        int base = 0;
        for (int i0 = 0; i0 < n; i0 += EM_SHRINK_THREADS) {
            int32_t v[EM_SHRINK_THREADS];
            unsigned long long mask[NW] = {};
            int cnt[NW] = {};
            for (int tid = 0; tid < EM_SHRINK_THREADS; ++tid) {          // every thread reads, then the barrier
                const int i = i0 + tid;
                v[tid] = i < n ? list[i] : 0;
                if (i < n && status[v[tid]] != 2) mask[tid >> 6] |= 1ull << (tid & 63);
            }
            for (int w = 0; w < NW; ++w) cnt[w] = __builtin_popcountll(mask[w]);
            for (int tid = 0; tid < EM_SHRINK_THREADS; ++tid)
                if (mask[tid >> 6] >> (tid & 63) & 1ull) {
                    const int pos = em_shrink_pos(base, cnt, tid >> 6, mask[tid >> 6], tid & 63);
                    CHECK(pos >= 0 && pos <= i0 + tid, "entry %d moves up to %d", i0 + tid, pos);
                    if (pos >= 0 && pos <= i0 + tid) list[pos] = v[tid];
                }
            for (int w = 0; w < NW; ++w) base += cnt[w];
        }
        CHECK(base == (int)expect.size() && std::equal(expect.begin(), expect.end(), list.begin()), "compaction of %d entries, mode %d", n, mode);
    }
    printf("shrink: %d slot cases, %d grid and compaction cases\n", n_cases * 20, n_cases);
}

int main() {
    std::mt19937_64 rng(20261018);
    check_schedules(rng, 200000);
    check_plans(rng, 3000);
    check_shrink(rng, 3000);
    if (g_fail) {
        fprintf(stderr, "%d checks FAILED\n", g_fail);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
