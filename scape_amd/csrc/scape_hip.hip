// scape_hip.hip - gfx950 (MI355X) kernels + C ABI for SCAPE's infer_pa hot path.
//
// What is computed is specified by the reference's Python (citations: /root/reference/src/scape/):
//   Phase A  point log-likelihoods        taichi_core.py:101-157, apa_core.py:954-957
//   Phase B  marginal tensor over (a, b)  taichi_core.py:160-246
//   EM       em_algo / mstep / elbo / bic apa_core.py:473-573, :702-779
//   labels   get_label                    apa_core.py:873-881
// How it is computed is MI355X-first: every array keeps the bin axis (n) fastest so that the
// 64 lanes of a wavefront read/write consecutive f64; rows are padded to a 16-element pitch so
// rows start 128-B aligned and can be read as double2.  The EM advances all (UTR, K, restart) jobs of a call
// in lock-step rounds (em_lockstep.inc): k2_estep, one wavefront per job (responsibilities, weights, ELBO),
// then an M-step kernel (mstep.inc), one workgroup per (UTR, 64-row tensor tile), which multiplies the tile with the v vectors of
// every job whose window covers it on the f64 matrix cores and keeps per-(job, tile) first arg-maxes.
// All arithmetic is f64 (the reference's finite -inf sentinel overflows f32).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <chrono>
#include <utility>
#include <vector>

#include "scape_hip.h"

#define SENT SCAPE_SENT
#define PI_REF 3.141592653589793  // taichi_core.py:9
#define PITCH 16                  // row pitch granule (f64 elements) -> 128-B aligned rows
#define TILE_ROWS 64               // tensor rows per M-step tile (= MT_ROWS of em_lockstep.inc)

// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(const std::string &msg) {
    g_err = msg;
    return 1;
}
#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(std::string(#expr) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + \
                        ":" + std::to_string(__LINE__) + ")");                               \
    } while (0)

// ------------------------------------------------------------------------------------------
// device-side descriptors
// ------------------------------------------------------------------------------------------
struct UtrDesc {
    int64_t bin_off;    // first bin in x/l/r/pa/cnt
    int64_t theta_off;  // first grid point in theta
    int64_t at_off;     // offset (f64) of AT / V  [T][Np]
    int64_t m_off;      // offset (f64) of M       [T][B][Np]
    int64_t log_off;    // first entry in the log-domain bin list
    int64_t tile_off;   // first entry of this UTR in the per-tile extent table (64-row tiles of M)
    int64_t mlog_off;   // first entry of this UTR in the compact table of log-domain values (phase_b.inc)
    int32_t c_lo, c_hi; // uniform theta grid: the interior grid points [c_lo, c_hi] share one window table; c_lo > c_hi: none
    int32_t N, Np, T, n_log;
    double unif_ll, L, min_theta;
};

struct DevParams {
    double mu_f, sigma_f, max_unif_ws;
    int32_t B, S, nround, pad;
    double betas[SCAPE_MAX_BETA];
    double s_dis[SCAPE_MAX_S];
    double pmf_s[SCAPE_MAX_S];
    double inv_s[SCAPE_MAX_S];   // 1 / s_dis[j] (the same IEEE quotient the kernels would compute per bin)
};

// ------------------------------------------------------------------------------------------
// device functions: the reference's @ti.func set (taichi_core.py:24-97)
// ------------------------------------------------------------------------------------------
// log(x) for finite x > 0 (subnormals included) in ~35 f64 instructions instead of the ~85 of the library's
// double-double routine - the tensor build takes one log per entry (13 x N x T per UTR) and is bound by them.
// Algorithm: the classic argument reduction x = 2^k (1+f), sqrt(2)/2 <= 1+f < sqrt(2), s = f/(2+f),
// log(1+f) = f - hfsq + s (hfsq + R(s^2)) with the degree-14 minimax R in s (coefficients Lg1..Lg7, error < 2^-58.45),
// k ln2 added as a hi/lo pair; the quotient comes from v_rcp_f64 plus two Newton steps and a residual correction.
// Worst error found on 2e7 arguments (host replica of exactly this sequence, against long-double log): 0.83 ulp.
// The polynomial constants of d_log_pos / d_exp_nonpos as a caller may hold them.  Left to the compiler (the default
// argument: plain literals) every Horner step inside a big loop becomes v_mov_b64 (a fresh copy of the addend constant) +
// v_fmac_f64.  A loop that is bound by its VALU count (the E-step's bin loop) takes d_*_poly_held() in front of the loop
// instead: the multiplier-side constants sit in scalar registers, the addend-side ones in vector registers the compiler
// cannot re-create, and each step is one three-address v_fma_f64.  Same operations, same order, same bits.
struct LogPoly {
    double Lg1, Lg2, Lg3, Lg4, Lg5, Lg6, Lg7;
};
struct ExpPoly {
    double c5, c4, c3;
};
#define D_LOG_POLY LogPoly{6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01, \
                           1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01}
#define D_EXP_POLY ExpPoly{1.0 / 120, 1.0 / 24, 1.0 / 6}
__device__ __forceinline__ LogPoly d_log_poly_held() {
    LogPoly k = D_LOG_POLY;
    asm volatile("" : "+s"(k.Lg1), "+s"(k.Lg2), "+s"(k.Lg3), "+s"(k.Lg6), "+s"(k.Lg7));   // multipliers, last addends
    asm volatile("" : "+v"(k.Lg4), "+v"(k.Lg5));                                            // addends of the innermost steps
    return k;
}
__device__ __forceinline__ ExpPoly d_exp_poly_held() {
    ExpPoly k = D_EXP_POLY;
    asm volatile("" : "+s"(k.c5), "+s"(k.c3));
    asm volatile("" : "+v"(k.c4));
    return k;
}
__device__ __forceinline__ double d_log_pos(double x, const LogPoly &k = D_LOG_POLY) {
#pragma clang fp contract(off)
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10,
                 Lg1 = k.Lg1, Lg2 = k.Lg2, Lg3 = k.Lg3, Lg4 = k.Lg4, Lg5 = k.Lg5, Lg6 = k.Lg6, Lg7 = k.Lg7;
    double m = __builtin_amdgcn_frexp_mant(x);        // [0.5, 1)
    int e = __builtin_amdgcn_frexp_exp(x);
    const bool lo = m < 0.70710678118654752440;
    m = lo ? m * 2.0 : m;
    e = lo ? e - 1 : e;
    const double f = m - 1.0, d = 2.0 + f;
    double r = __builtin_amdgcn_rcp(d);
    r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
    double s = f * r;
    s = __builtin_fma(__builtin_fma(-d, s, f), r, s);
    const double dk = (double)e, z = s * s, w = z * z;
    const double t1 = w * __builtin_fma(w, __builtin_fma(w, Lg6, Lg4), Lg2);
    const double t2 = z * __builtin_fma(w, __builtin_fma(w, __builtin_fma(w, Lg7, Lg5), Lg3), Lg1);
    const double R = t2 + t1;
    const double hfsq = 0.5 * f * f;
    const double inner = __builtin_fma(s, hfsq + R, dk * ln2_lo);
    return dk * ln2_hi - ((hfsq - inner) - f);
}

#include "exp_table.inc"
// exp(x) for x <= 0 in ~18 f64 instructions + one 16-byte LDS read (the library routine takes ~37): the E-step
// takes one exp per (bin, component, round), Phase A thirteen per (bin, theta) - both are bound by them.
// x = (128 e + j) ln2/128 + r, |r| <= ln2/256: exp(x) = 2^e * T[j] * (1 + p(r)), T[j] = 2^(j/128) as a hi/lo pair
// (table in LDS: d_load_exptab), p = expm1 to degree 5 (next term r^6/720 < 2^-62).  Arguments below -750 give 0
// like exp itself.  Worst error on 3e7 arguments in [-700, 0] (host replica, against long-double exp): 0.60 ulp.
__device__ __forceinline__ void d_load_exptab(double2 *tab /* LDS, 128 entries */, int tid, int nthreads) {
    for (int i = tid; i < 128; i += nthreads) tab[i] = g_exp_tab[i];
}
__device__ __forceinline__ double d_exp_nonpos(double x, const double2 *tab, const ExpPoly &k = D_EXP_POLY) {
#pragma clang fp contract(off)
    x = fmax(x, -750.0);
    const double n = __builtin_rint(x * EXP_INV_L);
    double r = __builtin_fma(n, -EXP_L_HI, x);
    r = __builtin_fma(n, -EXP_L_LO, r);
    const int ni = (int)n;
    const double2 t = tab[ni & 127];
    const double r2 = r * r;
    const double q = __builtin_fma(r, __builtin_fma(r, __builtin_fma(r, k.c5, k.c4), k.c3), 0.5);
    const double p = __builtin_fma(r2, q, r);
    return ldexp(t.x + __builtin_fma(t.x, p, t.y), ni >> 7);
}

// 1/x for x in [2^-20, 2^20] (no scaling or special cases needed): v_rcp_f64 + two Newton steps, within an ulp of the quotient
__device__ __forceinline__ double d_rcp_mid(double x) {
#pragma clang fp contract(off)
    double r = __builtin_amdgcn_rcp(x);
    r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
    return r;
}

__device__ __forceinline__ double d_logw(double w) { return (w <= 0.0) ? SENT : log(w); }

// cal_bic (apa_core.py:702-706).  The product and the sum are rounded one after the other, as numpy rounds them: left to
// the compiler, some instantiations of the E-step (a compile-time K in one, a run-time K in the other) fused them into
// one FMA and others did not, and the same job came back with a BIC one ulp apart depending on the column class of the
// call it was part of (tests/test_em_column_classes.py)
__device__ __forceinline__ double d_bic(double ell, int K, int N) {
#pragma clang fp contract(off)
    const double penalty = (double)(3 * K + 1) * log((double)N);
    return -2.0 * ell + penalty;
}
__device__ __forceinline__ double d_logpdf_normal(double x, double mu, double sigma) {
    double z = (x - mu) / sigma;
    return -0.5 * (z * z) - log(sigma) - 0.5 * log(2 * PI_REF);
}
__device__ __forceinline__ double d_pdf_normal(double x, double mu, double sigma) {
    double z = (x - mu) / sigma;
    return exp(-0.5 * (z * z)) / sqrt(2 * PI_REF) / sigma;
}

__device__ __forceinline__ double d_pdf_normal_t(double x, double mu, double sigma, const double2 *tab) {
    double z = (x - mu) / sigma;
    return d_exp_nonpos(-0.5 * (z * z), tab) / sqrt(2 * PI_REF) / sigma;
}

// loglik_xlr_t_pa_kernel body (taichi_core.py:101-107)
__device__ __forceinline__ double d_point_pa(double x, double l, double pa, double th, double sigma_f) {
    double u = th - x;
    double ll_l = (l <= u) ? -log(u) : SENT;
    return ll_l + d_logpdf_normal(pa - th, 0.0, sigma_f);
}
// loglik_xlr_t_r_unknown_kernel body (taichi_core.py:141-157); returns v (linear), A through *a
__device__ __forceinline__ double d_point_r_unknown(double x, double l, double th, const double *s,
                                                    const double *pmf, const double *inv_s, int S, double mu_f,
                                                    double sigma_f, double *a, const double2 *tab) {
    double u = th - x;
    double v = 0.0;
    if (l <= u) {  // lik_l_xt == 0 otherwise, every term of the sum is then exactly 0
        // 1/s_j * pdfN(x; th + s_j - mu_f, sigma_f) * lk * pmf_j, summed in j order.  The reference divides four times
        // per term (1/s_j, z = ./sigma, /sqrt(2 pi), /sigma); here the three divisors that do not depend on the bin
        // become reciprocals taken once (each product then differs from the quotient by at most an ulp: 4e-16 relative
        // on v, against the 1e-13 the log-domain comparison with the reference allows) - 52 divisions of ~14
        // instructions per (bin, theta) were three quarters of this kernel
        const double lk = 1 / u, inv_sigma = 1 / sigma_f, inv_norm = 1 / sqrt(2 * PI_REF);
        for (int j = 0; j < S; ++j) {
            const double z = (x - (th + s[j] - mu_f)) * inv_sigma;
            const double pdf = d_exp_nonpos(-0.5 * (z * z), tab) * inv_norm * inv_sigma;
            v += inv_s[j] * pdf * lk * pmf[j];
        }
    }
    if (v < 1e-300) v = 0.0;
    *a = (v <= 0.0) ? SENT : d_log_pos(v);
    return v;
}
// loglik_xlr_t_r_known_kernel body (taichi_core.py:111-132), two-pass logsumexp (:40-54)
__device__ __forceinline__ double d_point_r_known(double x, double l, double r, double th,
                                                  const double *s, const double *pmf, int S,
                                                  double mu_f, double sigma_f) {
    double u = th - x;
    double ll_l = (l <= u) ? -log(u) : SENT;
    double tmpn = 0.0, mx = 0.0;
    for (int j = 0; j < S; ++j) {
        double t;
        if (s[j] < r) {
            t = SENT;
        } else {
            tmpn += pmf[j];
            double lrs = (r <= s[j]) ? -log(s[j]) : SENT;
            t = lrs + d_logpdf_normal(x, th + s[j] - mu_f, sigma_f) + ll_l + log(pmf[j]);
        }
        if (j == 0 || t > mx) mx = t;
    }
    double sum = 0.0;
    for (int j = 0; j < S; ++j) {
        double t;
        if (s[j] < r) {
            t = SENT;
        } else {
            double lrs = (r <= s[j]) ? -log(s[j]) : SENT;
            t = lrs + d_logpdf_normal(x, th + s[j] - mu_f, sigma_f) + ll_l + log(pmf[j]);
        }
        sum += exp(t - mx);
    }
    return log(sum) + mx - log(tmpn);
}

// np.sum over a short contiguous f64 run, in numpy's own order (sequential below 8 elements,
// 8 interleaved accumulators above) so that row normalisations round like the reference's
template <int CMAX>
__device__ __forceinline__ double d_np_sum(const double (&a)[CMAX], int C) {
    if (C < 8) {
        double r = 0.0;
#pragma unroll
        for (int i = 0; i < (CMAX < 7 ? CMAX : 7); ++i)
            if (i < C) r += a[i];
        return r;
    }
    if constexpr (CMAX >= 8) {
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        const int lim = C - (C % 8);
#pragma unroll
        for (int i = 8; i + 8 <= CMAX; i += 8)
            if (i < lim) {
#pragma unroll
                for (int j = 0; j < 8; ++j) r[j] += a[i + j];
            }
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
        for (int i = 8; i < CMAX; ++i)
            if (i >= lim && i < C) res += a[i];
        return res;
    }
    return 0.0;
}

// ------------------------------------------------------------------------------------------
// operator-level kernels (the taichi_core seam: one theta, one data subset)
// ------------------------------------------------------------------------------------------
__global__ void k_op_pa(const double *x, const double *l, const double *pa, int n, double theta,
                        double sigma_f, double *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = d_point_pa(x[i], l[i], pa[i], theta, sigma_f);
}
__global__ void k_op_r_known(const double *x, const double *l, const double *r, int n, DevParams P,
                             double theta, double *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = d_point_r_known(x[i], l[i], r[i], theta, P.s_dis, P.pmf_s, P.S, P.mu_f, P.sigma_f);
}
__global__ void k_op_r_unknown(const double *x, const double *l, int n, DevParams P, double theta,
                               double *out) {
    __shared__ double2 s_exptab[128];
    d_load_exptab(s_exptab, threadIdx.x, blockDim.x);
    __syncthreads();
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        double a;
        d_point_r_unknown(x[i], l[i], theta, P.s_dis, P.pmf_s, P.inv_s, P.S, P.mu_f, P.sigma_f, &a, s_exptab);
        out[i] = a;
    }
}

// ------------------------------------------------------------------------------------------
// Phase A: AT[t][n] = log p(bin n | theta_t) and V[t][n] = p(bin n | theta_t) (linear domain,
// r-unknown bins only).  grid = (ceil(Np/256), T_max, n_utr); n is the lane axis.
// ------------------------------------------------------------------------------------------
#define PA_TT 8      // theta grid points per workgroup: the bin's data, the UTR descriptor and the exp table are fetched once for all of them
__global__ __launch_bounds__(256) void k_phase_a(const UtrDesc *__restrict__ descs, DevParams P,
                                                 const double *__restrict__ x,
                                                 const double *__restrict__ l,
                                                 const double *__restrict__ r,
                                                 const double *__restrict__ pa,
                                                 const double *__restrict__ theta,
                                                 double *__restrict__ AT, double *__restrict__ V) {
    __shared__ double2 s_exptab[128];
    d_load_exptab(s_exptab, threadIdx.x, blockDim.x);
    __syncthreads();
    const UtrDesc d = descs[blockIdx.z];
    const int t0 = blockIdx.y * PA_TT, t1 = min(d.T, t0 + PA_TT);
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (t0 >= d.T || n >= d.Np) return;
    if (n >= d.N) {
        for (int t = t0; t < t1; ++t) {
            const size_t o = (size_t)d.at_off + (size_t)t * d.Np + n;
            AT[o] = 0.0;
            V[o] = 0.0;
        }
        return;
    }
    const double xn = x[d.bin_off + n], ln = l[d.bin_off + n];
    const double rn = r[d.bin_off + n], pan = pa[d.bin_off + n];
    for (int t = t0; t < t1; ++t) {
        const size_t o = (size_t)d.at_off + (size_t)t * d.Np + n;
        const double th = theta[d.theta_off + t];
        double a, v = 0.0;
        if (!isnan(pan)) {
            a = d_point_pa(xn, ln, pan, th, P.sigma_f);
        } else if (!isnan(rn)) {
            a = d_point_r_known(xn, ln, rn, th, P.s_dis, P.pmf_s, P.S, P.mu_f, P.sigma_f);
        } else {
            v = d_point_r_unknown(xn, ln, th, P.s_dis, P.pmf_s, P.inv_s, P.S, P.mu_f, P.sigma_f, &a, s_exptab);
        }
        AT[o] = a;
        V[o] = v;
    }
}

#include "phase_b.inc"      // Phase B: M[i][j][n], the marginal tensor over (alpha_i, beta_j) - all three forms
#include "em_lockstep.inc"  // the E-step, the shrink kernel and the EM's shared constants
#include "mstep.inc"        // the M-step: the frame its three kernels share, then k2_mstep, k3_mstep, k4_mstep
#include "mstep_staged.inc"
#include "mstep_ring.inc"
#include "mstep_multi.inc"

// ------------------------------------------------------------------------------------------
// labels: get_label (apa_core.py:873-881), one workgroup per selected model
// ------------------------------------------------------------------------------------------
template <int CMAX>
__global__ __launch_bounds__(256) void k_labels(const UtrDesc *__restrict__ descs, DevParams P,
                                                const double *__restrict__ cnt,
                                                const double *__restrict__ M, int kmax,
                                                const int32_t *__restrict__ sel_utr,
                                                const int32_t *__restrict__ sel_K,
                                                const int32_t *__restrict__ a_in,
                                                const int32_t *__restrict__ b_in,
                                                const double *__restrict__ ws_in,
                                                int32_t *__restrict__ labels) {
    __shared__ double2 s_exptab[128];
    d_load_exptab(s_exptab, threadIdx.x, blockDim.x);
    __syncthreads();
    const int sel = blockIdx.x;
    const UtrDesc d = descs[sel_utr[sel]];
    const int K = sel_K[sel], C = K + 1, B = P.B;
    const double *Mu = M + (size_t)d.m_off;
    size_t roff[CMAX];
    double slw[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        roff[c] = (c < K) ? ((size_t)a_in[(size_t)sel * kmax + c] * B + b_in[(size_t)sel * kmax + c]) * d.Np : 0;
        slw[c] = (c < C) ? d_logw(ws_in[(size_t)sel * (kmax + 1) + c]) : 0.0;
    }
    for (int n = threadIdx.x; n < d.N; n += blockDim.x) {
        const double cn = cnt[d.bin_off + n];
        double lz[CMAX], z[CMAX], mx = 0.0;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            if (c < C) {
                lz[c] = (c < K) ? slw[c] + Mu[roff[c] + n] : slw[c] + d.unif_ll;
                mx = (c == 0 || lz[c] > mx) ? lz[c] : mx;
            } else {
                lz[c] = 0.0;
            }
        }
#pragma unroll
        for (int c = 0; c < CMAX; ++c) z[c] = (c < C) ? d_exp_nonpos((lz[c] - mx) * cn, s_exptab) : 0.0;
        const double s = d_np_sum<CMAX>(z, C);
        int best = 0;
        double bz = 0.0;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            const double zc = z[c] / s;
            if (c < C && (c == 0 || zc > bz)) {
                bz = zc;
                best = c;
            }
        }
        labels[d.bin_off + n] = best;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// scape_hip_ctx is the handle: stream, error word, counters, timing events, report state.  What lives as long as a loaded
// batch is one BatchState that the handle owns and scape_hip_batch_free / scape_hip_destroy reset; its buffers are
// DevBufs, which free themselves, so nothing keeps a release list.  The entry points are built from host-only halves
// that make no HIP call (batch_plan, phase_b_choose, em_jobs_check, labels_check, em_plan: tools/batch_plan_check.cpp and
// tools/em_schedule_check.cpp drive them on the CPU) and from the steps allocate / upload / launch / download; the ones
// that queue copies on the caller's memory keep the drain rule (StreamDrain below).
//
// owns its device memory: freed when the buffer goes, so whoever holds one by value needs no release list
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t bytes) {
        if (bytes <= cap && p) return 0;
        // a buffer that has to grow gets 1/8 headroom: successive batches of a stream differ by a few per cent in
        // size, and re-allocating tens of GB for each of them costs more than the batch itself
        // (large buffers get it from the start: device memory costs ~25 ms per GB to allocate, and the second batch of a
        // stream is a few per cent larger than the first as often as not)
        // - not the very large ones: engines that share a device size their batches to a fraction of what is free, and
        //   12 % on top of each pushed two worker processes on one GPU over the edge (one of them ran 3x slower)
        const bool regrow = p != nullptr || (bytes > ((size_t)1 << 30) && bytes <= ((size_t)48 << 30));
        if (p) {
            (void)hipFree(p);
            p = nullptr;
            cap = 0;
        }
        if (bytes == 0) bytes = 16;
        size_t want = regrow ? bytes + bytes / 8 : bytes;
        if (hipMalloc(&p, want) != hipSuccess) {     // no room for the headroom: exact size
            (void)hipGetLastError();
            p = nullptr;
            want = bytes;
            HIPCHK(hipMalloc(&p, want));
        }
        cap = want;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T>
    T *as() const {
        return reinterpret_cast<T *>(p);
    }
};
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value,
              "a copy of a DevBuf would free its memory twice");

// One rule for every entry point that queues a copy from or into memory it does not own (the caller's arrays, host
// vectors of its own): once it has queued anything on the stream it returns, with 0 or with 1, only after the stream has
// been waited for.  StreamDrain keeps it: armed before the first queueing, it waits when it goes out of scope unless
// wait() has done so.  Host memory that a queued copy reads or writes outlives that wait: it is the caller's, or it is
// declared ahead of the drain (in perm.inc: in the base of a test's frame, RepPermHost goes after RepPermCall's drain).
// The one exception is scape_hip_batch_build: it queues by design, touches no caller memory, and finish_build reads its flag.
struct StreamDrain {
    hipStream_t stream;
    bool armed;
    explicit StreamDrain(hipStream_t s, bool a = true) : stream(s), armed(a) {}
    StreamDrain(const StreamDrain &) = delete;
    StreamDrain &operator=(const StreamDrain &) = delete;
    int wait() { armed = false; HIPCHK(hipStreamSynchronize(stream)); return 0; }
    ~StreamDrain() { if (armed) (void)hipStreamSynchronize(stream); }
};

struct EventPair {
    hipEvent_t a, b;
};

struct ReportState;   // report.inc

// Device buffers of the lock-step EM (em_lockstep.inc): the per-job state the kernels see as an EmState, the index
// tables of a call's plan (EmPlan) and the debug histogram of SCAPE_HIP_DEBUG.
struct EmBufs {
    DevBuf ia, ib, sia, sib, ws, slw, lb, ell, nlb, status, pend, rd_k, rd_lo, rd_hi, rd_m, rd_n0, rd_n1, rd_lw, rd_sv, rd_fl, V, Vsuf,
        voff, pt_score, pt_row, ptoff;             // one per EmState member, in its order
    DevBuf ujoff, ujlist, active, elist, dbg;
    DevBuf udone, shrunk;                          // em_rounds' shrink: finalised jobs per UTR; what k_em_shrink kept (3 ints)
    // nc = column slots of the call (jobs x depth): what the M-step reads and writes is per column
    int ensure(size_t nj, size_t nc, size_t kmax, size_t n_utr, size_t vtot, size_t pttot) {
        return ia.ensure(nj * kmax * 4) || ib.ensure(nj * kmax * 4) || sia.ensure(nj * kmax * 4) || sib.ensure(nj * kmax * 4) ||
               ws.ensure(nj * (kmax + 1) * 8) || slw.ensure(nj * (kmax + 1) * 8) || lb.ensure(nj * 8) || ell.ensure(nj * 8) ||
               nlb.ensure(nj * 4) || status.ensure(nj * 4) || pend.ensure(nj * 8) || rd_k.ensure(nc * 4) || rd_lo.ensure(nc * 4) ||
               rd_hi.ensure(nc * 4) || rd_m.ensure(nc * 4) || rd_n0.ensure(nc * 4) || rd_n1.ensure(nc * 4) ||
               rd_lw.ensure(nc * 8) || rd_sv.ensure(nc * 8) || rd_fl.ensure(nc * 8) || V.ensure(vtot * 8) || Vsuf.ensure((vtot / 16 + nc + 1) * 8) ||
               voff.ensure(nc * 8) || pt_score.ensure(pttot * 8) || pt_row.ensure(pttot * 4) || ptoff.ensure(nc * 8) ||
               ujoff.ensure((n_utr + 1) * 8) || ujlist.ensure(nc * 4) || active.ensure(n_utr * 4) || elist.ensure(nj * 4) ||
               udone.ensure(n_utr * 4) || shrunk.ensure(4 * 4);
    }
    EmState state(bool count_done = false) const {
        return EmState{ia.as<int32_t>(), ib.as<int32_t>(), sia.as<int32_t>(), sib.as<int32_t>(), ws.as<double>(), slw.as<double>(),
                       lb.as<double>(), ell.as<double>(), nlb.as<int32_t>(), status.as<int32_t>(), pend.as<unsigned long long>(),
                       rd_k.as<int32_t>(),
                       rd_lo.as<int32_t>(), rd_hi.as<int32_t>(), rd_m.as<int32_t>(), rd_n0.as<int32_t>(), rd_n1.as<int32_t>(),
                       rd_lw.as<double>(), rd_sv.as<double>(), rd_fl.as<double>(), V.as<double>(), Vsuf.as<double>(), voff.as<int64_t>(),
                       pt_score.as<double>(), pt_row.as<int32_t>(), ptoff.as<int64_t>(), count_done ? udone.as<int32_t>() : nullptr};
    }
};

// one queued copy to / from a DevBuf
static int to_dev(hipStream_t s, const DevBuf &d, const void *src, size_t bytes) {
    HIPCHK(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, s));
    return 0;
}
static int to_host(hipStream_t s, void *dst, const DevBuf &d, size_t bytes) {
    HIPCHK(hipMemcpyAsync(dst, d.p, bytes, hipMemcpyDeviceToHost, s));
    return 0;
}

// The job tables of scape_hip_batch_em, which sizes, uploads and downloads them: what the caller hands in, what it gets
// back, and the rows that scape_hip_batch_em_fetch_lb gathers from lb afterwards.
struct JobBufs {
    DevBuf utr, K, fixed, a, b, ws, karr, ao, bo, wso, bic, nlb, lb, sel, lbsel;
};
// The model tables of scape_hip_batch_labels and the labels of every bin of the batch.
struct LabelBufs {
    DevBuf utr, K, a, b, ws, labels;
};

// What batch_plan (host only) works out of a batch's arrays: the per-UTR descriptors and the totals, maxima and Phase B
// facts that the allocation, the build and the EM driver size themselves by.
struct BatchShape {
    int n_utr = 0, T_max = 0, Np_max = 0, W_max = 1, tiles_max_all = 1;
    int64_t n_bins = 0;
    std::vector<UtrDesc> h_desc;
    size_t at_total = 0, m_total = 0, tiles_total = 0, n_theta_total = 0, mlog_total = 0, n_logbins = 0;
    bool pb_slide = false;            // every UTR of the batch has a uniform theta grid with interior points: k_pb_logcol / k_pb_slide
};
struct BatchPlan : BatchShape {
    std::vector<int32_t> loglist, logbin_utr;   // uploaded by the load, not kept: log-domain bins by UTR, and the UTR of each
};

// Everything with the lifetime of a loaded batch.  The handle owns one (scape_hip_ctx::batch): scape_hip_batch_load
// makes it on first use and reuses its buffers from then on (DevBuf::ensure's headroom is there for the engine's wave
// after wave), scape_hip_batch_free and scape_hip_destroy reset it, and every DevBuf in it frees itself.
struct BatchState : BatchShape {
    DevParams prm;
    bool loaded = false, built = false;
    bool build_unchecked = false;     // Phase A/B are queued, their device-side consistency flag has not been read yet
    int pb_form = 0;                  // Phase B form of the last batch_build (scape_hip_batch_phase_b_form)
    int last_em_jobs = 0;             // jobs of the last completed scape_hip_batch_em call (scape_hip_batch_em_fetch_lb)
    DevBuf d_x, d_l, d_r, d_pa, d_cnt, d_theta, d_desc, d_loglist, d_AT, d_V, d_M, d_tile_nend;
    DevBuf d_tbi, d_tbG, d_tbpm, d_mlog, d_logbin;   // Phase B: window tables, compact log-domain values, log bin -> UTR
    JobBufs job;
    LabelBufs lab;
    EmBufs em;
};

#define N_COUNTERS (4 + 5 * 64 + 16 + 48)   // (+16: ESTEP_STAMPS, +48: M4_STAMPS tools builds) rounds, unused, z elements, finalised jobs, then five 64-way sharded counters (em_lockstep.inc)
// What lives as long as the handle; the batch hangs off it.
struct scape_hip_ctx {
    int device = 0;
    std::atomic<bool> busy{false};   // a handle serves one host thread at a time (scape_hip.h)
    hipStream_t stream = nullptr;
    char name[256] = {0};
    std::unique_ptr<BatchState> batch;   // null until the first scape_hip_batch_load and after scape_hip_batch_free
    DevBuf d_err, d_counters;
    std::vector<EventPair> ev[6];
    double ms_acc[6] = {0, 0, 0, 0, 0, 0};
    int n_acc[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long h_counters[3] = {0, 0, 0};
    unsigned long long h_traffic[4] = {0, 0, 0, 0};   // last EM call: M-step tensor bytes, v bytes requested / unique, launches
    ReportState *rep = nullptr;       // count-matrix / expected-length buffers (report.inc), made on first use
};

static int ev_begin(scape_hip_ctx *c, int which) {
    EventPair e;
    HIPCHK(hipEventCreate(&e.a));
    HIPCHK(hipEventCreate(&e.b));
    HIPCHK(hipEventRecord(e.a, c->stream));
    c->ev[which].push_back(e);
    return 0;
}
static int ev_end(scape_hip_ctx *c, int which) {
    HIPCHK(hipEventRecord(c->ev[which].back().b, c->stream));
    return 0;
}
static int ev_collect(scape_hip_ctx *c) {
    HIPCHK(hipStreamSynchronize(c->stream));
    const bool trace = getenv("SCAPE_HIP_ROUND_TRACE") != nullptr;   // per-launch durations on stderr
    for (int w = 0; w < 6; ++w) {
        int i = 0;
        for (auto &e : c->ev[w]) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, e.a, e.b));
            if (trace && w >= 4) fprintf(stderr, "[trace] kind %d launch %d %.4f ms\n", w, i, ms);
            ++i;
            c->ms_acc[w] += ms;
            c->n_acc[w] += 1;
            (void)hipEventDestroy(e.a);
            (void)hipEventDestroy(e.b);
        }
        c->ev[w].clear();
    }
    return 0;
}

static int round_up(int v, int g) { return (v + g - 1) / g * g; }

static int set_device(scape_hip_ctx *c) {
    HIPCHK(hipSetDevice(c->device));
    return 0;
}

// Calls on one handle are not re-entrant: a second host thread entering while a call is in flight gets an
// error instead of racing on the handle's device buffers.
struct BusyGuard {
    scape_hip_ctx *c;
    bool ok;
    explicit BusyGuard(scape_hip_ctx *ctx) : c(ctx), ok(ctx && !ctx->busy.exchange(true)) {}
    ~BusyGuard() { if (ok) c->busy.store(false); }
};
#define CTX_GUARD(c)                                                                                      \
    if (!(c)) return fail("ctx is NULL");                                                                 \
    BusyGuard busy_guard_(c);                                                                             \
    if (!busy_guard_.ok) return fail("handle is in use by another host thread (calls on a handle are not re-entrant)")
#define CTX_ENTER(c)                                                                                      \
    CTX_GUARD(c);                                                                                         \
    if (set_device(c)) return 1
// the first lines of an entry point that works on the built batch: the guard, then `b`, the handle's batch
#define BUILT_BATCH(c, b)                                                                                 \
    CTX_GUARD(c);                                                                                         \
    if (!(c)->batch || !(c)->batch->built) return fail("batch_build has not run");                        \
    BatchState &b = *(c)->batch

static void fill_params(DevParams &d, double mu_f, double sigma_f, double max_unif_ws, int B,
                        const double *betas, int S, const double *s, const double *pmf, int nround) {
    memset(&d, 0, sizeof(d));
    d.mu_f = mu_f;
    d.sigma_f = sigma_f;
    d.max_unif_ws = max_unif_ws;
    d.B = B;
    d.S = S;
    d.nround = nround;
    for (int i = 0; i < B; ++i) d.betas[i] = betas[i];
    for (int i = 0; i < S; ++i) {
        d.s_dis[i] = s[i];
        d.pmf_s[i] = pmf[i];
        d.inv_s[i] = 1 / s[i];
    }
}

// widest +-3*beta window (in grid points) over all grid points of one theta grid
static int max_window(const double *th, int T, double beta) {
    int best = 1, a = 0, b = 0;
    for (int i = 0; i < T; ++i) {
        const double lo = th[i] - 3 * beta, hi = th[i] + 3 * beta;
        while (a < i && th[a] < lo) ++a;
        if (b < i) b = i;
        while (b + 1 < T && th[b + 1] <= hi) ++b;
        best = std::max(best, b - a + 1);
    }
    return best;
}

// The Phase B a build queues and what its kernels need.  Form 0: k_phase_b (one kernel).  Form 1: tables + log bins,
// then the matrix path per alpha (measured, round 3: 10.2 + 10.9 ms against 15.0 for k_phase_b - the log path's gather of
// A[w][n] at a row pitch of 8.5 KB keeps the texture addresser busy).  Form 2: tables, log-bin columns, sliding windows.
// The three give the same bits.
struct PhaseB {
    int form, Wmax, WP;
    size_t lds;                          // form 0: k_phase_b
    size_t lds_t, lds_l, lds_c, lds_s;   // forms 1 and 2: k_pb_tables, k_phase_b_lin, k_pb_logcol, k_pb_slide
};
// `mode` is SCAPE_HIP_PHASE_B: "v2" asks for form 0, "split" for form 1; otherwise form 2 where every theta grid of the
// batch is uniform (slide), and form 0 where not or where n_beta > 16.  Host only.
static int phase_b_choose(int B, int W_max, int T_max, bool slide, const char *mode, PhaseB &ch) {
    const bool v2 = mode && strcmp(mode, "v2") == 0, split = mode && strcmp(mode, "split") == 0;
    const int Wmax = W_max, WP = ((Wmax + 3) & ~3) + 1;
    ch = PhaseB{0, Wmax, WP, 0, 0, 0, 0, 0};
    if (B <= 16 && !v2 && (split || slide)) {
        ch.form = split ? 1 : 2;
        ch.lds_t = ((size_t)B * Wmax + 16) * sizeof(double) + 32 * sizeof(int);
        ch.lds_l = ((size_t)16 * WP + 16 * PB_LOGCAP) * sizeof(double) + PB_LOGCAP * sizeof(int);
        ch.lds_c = ((size_t)((T_max + 1) & ~1) + (size_t)B * Wmax) * sizeof(double) + 16 * sizeof(int);
        ch.lds_s = ((size_t)16 * WP + 4 * PB_RING * 16) * sizeof(double);
        if (ch.lds_t > 60 * 1024 || ch.lds_l > 60 * 1024) return fail("Phase B: window table does not fit LDS (n_beta x window too large)");
        return 0;
    }
    ch.lds = ((size_t)2 * B * Wmax + B) * sizeof(double) + (size_t)2 * (B + 1) * sizeof(int) + (size_t)16 * WP * sizeof(double);
    if (ch.lds > 150 * 1024) return fail("Phase B: window table does not fit LDS (n_beta x window too large)");
    return 0;
}

// Queues the chosen Phase B on the buffers of `b`: a loaded batch, or the one UTR that
// scape_hip_get_loglik_marginal_tensor sets up for itself (all_log: every bin takes the log-domain path; only d_desc,
// d_theta, d_AT and d_M are there, the other pointers are null).
static int queue_phase_b(scape_hip_ctx *c, const BatchState &b, const PhaseB &ch, int all_log = 0) {
    const UtrDesc *desc = b.d_desc.as<UtrDesc>();
    const double *r = b.d_r.as<double>(), *pa = b.d_pa.as<double>(), *theta = b.d_theta.as<double>(), *AT = b.d_AT.as<double>(),
                 *V = b.d_V.as<double>();
    const int32_t *loglist = b.d_loglist.as<int32_t>();
    double *M = b.d_M.as<double>(), *mlog = b.d_mlog.as<double>(), *tbG = b.d_tbG.as<double>(), *tbpm = b.d_tbpm.as<double>();
    int32_t *tbi = b.d_tbi.as<int32_t>(), *tile_nend = b.d_tile_nend.as<int32_t>();
    if (c->d_err.ensure(sizeof(int))) return 1;
    HIPCHK(hipMemsetAsync(c->d_err.p, 0, sizeof(int), c->stream));
    const dim3 by_alpha((unsigned)(((b.n_utr + 7) / 8) * 8 * b.T_max));
    if (ch.form == 0) {
        if (b.prm.B <= 16)
            hipLaunchKernelGGL(k_phase_b<16>, by_alpha, dim3(256), ch.lds, c->stream, desc, b.prm, r, pa, theta, loglist, AT, V, M,
                               ch.Wmax, all_log, c->d_err.as<int>(), b.n_utr, b.T_max, tile_nend);
        else
            hipLaunchKernelGGL(k_phase_b<1>, by_alpha, dim3(256), ch.lds, c->stream, desc, b.prm, r, pa, theta, loglist, AT, V, M,
                               ch.Wmax, all_log, c->d_err.as<int>(), b.n_utr, b.T_max, tile_nend);
        HIPCHK(hipGetLastError());
        return 0;
    }
    const bool slide = ch.form == 2;
    hipLaunchKernelGGL(k_pb_tables<16>, dim3((unsigned)b.T_max, (unsigned)b.n_utr), dim3(PB_TAB_THREADS), ch.lds_t, c->stream, desc,
                       b.prm, theta, ch.Wmax, ch.WP, tbi, tbG, tbpm, c->d_err.as<int>(), b.T_max, slide ? nullptr : loglist, AT, M, mlog,
                       tile_nend);
    HIPCHK(hipGetLastError());
    if (slide) {
        if (b.n_logbins) {
            hipLaunchKernelGGL(k_pb_logcol, dim3((unsigned)b.n_logbins), dim3(256), ch.lds_c, c->stream, desc, b.prm, theta, loglist,
                               b.d_logbin.as<int32_t>(), AT, tbi, tbG, M, mlog, tile_nend, ch.Wmax);
            HIPCHK(hipGetLastError());
        }
        const int blocks_max = (b.Np_max + 63) / 64;
        hipLaunchKernelGGL(k_pb_slide, dim3((unsigned)(((b.n_utr + 7) / 8) * 8 * blocks_max)), dim3(256), ch.lds_s, c->stream, desc,
                           b.prm, r, pa, loglist, V, M, mlog, ch.WP, tbi, tbpm, b.n_utr, blocks_max, tile_nend);
    } else {
        hipLaunchKernelGGL(k_phase_b_lin, by_alpha, dim3(256), ch.lds_l, c->stream, desc, b.prm, r, pa, loglist, V, M, mlog, ch.WP, tbi,
                           tbpm, b.n_utr, b.T_max, tile_nend);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

static int check_err_flag(scape_hip_ctx *c, const char *what) {
    int flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, c->d_err.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (flag) return fail(std::string(what) + ": device-side consistency check failed (flag " + std::to_string(flag) + ")");
    return 0;
}

// reads the consistency flag of a queued batch_build (synchronises the stream); a build that failed it is no build
static int finish_build(scape_hip_ctx *c) {
    BatchState *b = c->batch.get();
    if (!b || !b->build_unchecked) return 0;
    b->build_unchecked = false;
    b->built = check_err_flag(c, "batch_build") == 0;
    return !b->built;
}

// ------------------------------------------------------------------------------------------
// host driver of the lock-step EM (kernels in em_lockstep.inc and, on the frame of mstep.inc, mstep_staged.inc, mstep_ring.inc, mstep_multi.inc)
// ------------------------------------------------------------------------------------------
// Column classes: the CMAX template arguments each kernel family is instantiated for.  A call runs in the first class
// that holds its kmax + 1 columns.
using EstepClasses = std::integer_sequence<int, 4, 8, 12, 16, 24, 32, 64>;   // k2_estep, k2_estep_all_rounds
using WideClasses = std::integer_sequence<int, 4, 8, 12, 16>;                // k2_estep_cs
using LabelClasses = std::integer_sequence<int, 8, 16, 32, 64>;              // k_labels

template <int... Cs>
constexpr int last_class(std::integer_sequence<int, Cs...>) {
    int last = 0;
    ((last = Cs), ...);
    return last;
}
static_assert(last_class(EstepClasses{}) == SCAPE_MAX_K + 1 && last_class(LabelClasses{}) == SCAPE_MAX_K + 1,
              "the largest class holds the largest kmax a call may have");
constexpr int WIDE_MAX_COLUMNS = last_class(WideClasses{});

// f(std::integral_constant<int, C>()) for the first class C >= columns; false if there is none
template <int... Cs, typename F>
static bool with_column_class(std::integer_sequence<int, Cs...>, int columns, F &&f) {
    return ((columns <= Cs && (f(std::integral_constant<int, Cs>()), true)) || ...);
}

// Index tables of one EM call: the M-step columns (job j owns columns j * depth .. j * depth + depth - 1, one per round it
// may run in a launch) grouped by UTR, the UTRs and jobs in launch order, ragged offsets of the column vectors and of the
// per-tile partials.  Host only.
struct EmPlan {
    std::vector<int64_t> ujoff, voff, ptoff;     // [n_utr + 1] first column of a UTR in ujlist; [columns] offsets into V / pt_*
    std::vector<int32_t> ujlist, active, elist;  // columns by UTR; UTRs with jobs (M-step grid order); jobs in E-step order
    size_t vtot = 0, pttot = 0;
    int depth = 1;                               // column slots per job
    int tiles_max = 1, max_cols_utr = 1;
    bool any_m = false;                          // fixed-inference jobs (mstep_fixed) have no grid arg-max
};

// tiles of the largest UTR of a list: the second factor of the M-step grid (em_plan, and em_rounds after a shrink)
static int em_tiles_max(const std::vector<UtrDesc> &h_desc, int B, const int32_t *utrs, int n) {
    int tiles_max = 1;
    for (int i = 0; i < n; ++i) tiles_max = std::max(tiles_max, (h_desc[utrs[i]].T * B + MT_ROWS - 1) / MT_ROWS);
    return tiles_max;
}

static EmPlan em_plan(const std::vector<UtrDesc> &h_desc, int B, size_t nj, const int32_t *job_utr, const int32_t *job_fixed,
                      bool size_order, int depth) {
    EmPlan p;
    const int n_utr = (int)h_desc.size();
    p.depth = depth;
    p.ujoff.assign(n_utr + 1, 0);
    p.ujlist.resize(nj * depth);
    for (size_t j = 0; j < nj; ++j) p.ujoff[job_utr[j] + 1] += depth;
    for (int u = 0; u < n_utr; ++u) p.ujoff[u + 1] += p.ujoff[u];
    {
        std::vector<int64_t> fill(p.ujoff.begin(), p.ujoff.end() - 1);
        for (size_t j = 0; j < nj; ++j)
            for (int q = 0; q < depth; ++q) p.ujlist[fill[job_utr[j]]++] = (int32_t)(j * depth + q);
    }
    // UTRs that have at least one job in this call, in index order: the M-step grid runs over this list, so a call
    // that touches a few UTRs of a large resident batch (reference-stream mode) still uses every XCD
    for (int u = 0; u < n_utr; ++u)
        if (p.ujoff[u + 1] > p.ujoff[u]) p.active.push_back(u);
    // Blocks are dealt round-robin over the 8 XCDs and the M-step gives XCD x the UTRs at positions x, x + 8, ... of this
    // list: sorted by tensor size, the 8 UTRs that are in flight side by side are of one size class (their tiles take
    // alike) and every XCD gets the same mix - in index order an XCD that drew the large UTRs finishes last while
    // the others idle.  Placement only: a UTR's results do not depend on where or next to what it runs.
    if (size_order)
        std::stable_sort(p.active.begin(), p.active.end(), [&](int32_t a, int32_t b) {
            const UtrDesc &da = h_desc[a], &db = h_desc[b];
            return (int64_t)da.T * da.Np > (int64_t)db.T * db.Np;
        });
    const int n_active = (int)p.active.size();
    for (int u : p.active) {
        p.max_cols_utr = std::max<int>(p.max_cols_utr, (int)(p.ujoff[u + 1] - p.ujoff[u]));
    }
    p.tiles_max = em_tiles_max(h_desc, B, p.active.data(), n_active);
    p.voff.resize(nj * depth);
    p.ptoff.resize(nj * depth);
    for (size_t j = 0; j < nj; ++j) {
        const UtrDesc &d = h_desc[job_utr[j]];
        for (int q = 0; q < depth; ++q) {
            p.voff[j * depth + q] = (int64_t)p.vtot;
            p.ptoff[j * depth + q] = (int64_t)p.pttot;
            p.vtot += (size_t)d.Np;
            p.pttot += (size_t)((d.T * B + MT_ROWS - 1) / MT_ROWS);
        }
        p.any_m = p.any_m || job_fixed[j] == 0;
    }
    // The E-step gives XCD x the x-th eighth of its job list: with the jobs of UTR active[x], active[x + 8], ... there,
    // every XCD gets the same mix of sizes, and the v vectors a UTR's jobs write are read by the M-step tiles of the same
    // UTR on the same XCD (L2; speed only).
    // Otherwise: the jobs by UTR.
    p.elist.reserve(nj);
    auto jobs_of = [&](int u) {
        for (int64_t q = p.ujoff[u]; q < p.ujoff[u + 1]; q += depth) p.elist.push_back(p.ujlist[q] / depth);
    };
    if (size_order && n_active >= 8) {
        for (int x = 0; x < 8; ++x)
            for (int k = x; k < n_active; k += 8) jobs_of(p.active[k]);
    } else {
        for (int u = 0; u < n_utr; ++u) jobs_of(u);
    }
    return p;
}

// the environment switches of the EM driver (diagnostics; none changes results: DESIGN.md section 7)
struct EmSwitches {
    bool size_order, debug, fine, mstep_v2, mstep_v3;
    int split_maxtiles, wide_maxjobs;
    int depth;          // SCAPE_HIP_EM_DEPTH: cap on the rounds a job runs per launch (1 = one round per tensor pass)
    bool shrink;        // SCAPE_HIP_EM_SHRINK=0: the launches of a call that runs ahead keep their first size
    int shrink_at;      // SCAPE_HIP_EM_SHRINK_AT: compact the lists when at most this percentage of them is live
    bool trace;         // SCAPE_HIP_ROUND_TRACE: one stderr line per shrink
};
static EmSwitches em_switches() {
    const char *env_m = getenv("SCAPE_HIP_MSTEP"), *env_r = getenv("SCAPE_HIP_SPLIT_MAXTILES"), *env_w = getenv("SCAPE_HIP_WIDE_MAXJOBS");
    EmSwitches s;
    s.size_order = !getenv("SCAPE_HIP_NO_SIZE_ORDER");
    s.debug = getenv("SCAPE_HIP_DEBUG") != nullptr;           // the tile / job histograms are k2 / k3 only
    s.fine = getenv("SCAPE_HIP_ROUND_TIMING") != nullptr;
    s.mstep_v2 = env_m && strcmp(env_m, "v2") == 0;
    s.mstep_v3 = env_m && strcmp(env_m, "v3") == 0;
    s.split_maxtiles = env_r ? atoi(env_r) : 1024;
    s.wide_maxjobs = env_w ? atoi(env_w) : 1024;
    const char *env_d = getenv("SCAPE_HIP_EM_DEPTH");
    s.depth = std::min(EM_DEPTH, std::max(1, env_d ? atoi(env_d) : EM_DEPTH));
    const char *env_s = getenv("SCAPE_HIP_EM_SHRINK"), *env_a = getenv("SCAPE_HIP_EM_SHRINK_AT");
    s.shrink = !(env_s && atoi(env_s) == 0);
    s.shrink_at = std::min(100, std::max(1, env_a ? atoi(env_a) : EM_SHRINK_AT));
    s.trace = getenv("SCAPE_HIP_ROUND_TRACE") != nullptr;
    return s;
}

struct EmKernels {
    bool wide;          // E-step: 4 wavefronts per job (k2_estep_cs)
    bool job_split;     // M-step: a tile's jobs cut into passes of 16 that separate workgroups take
    bool ring_mstep;    // k3_mstep (LDS-DMA rings, mstep_ring.inc) instead of the register-staged k2_mstep
    bool multi_mstep;   // k4_mstep (several tiles per workgroup, mstep_multi.inc) instead of k3_mstep
};
// Small calls run the 4-wavefront E-step, which keeps one round per launch (its arithmetic is the same template body)
static bool em_wide(const EmSwitches &sw, int n_jobs, int kmax) {
    const bool wide = n_jobs <= sw.wide_maxjobs && kmax + 1 <= WIDE_MAX_COLUMNS;
    return wide;
}

// Column slots per job of a call: the switch's cap, 1 where nothing runs ahead (the 4-wavefront E-step of small calls,
// calls of fixed-inference jobs only), and no more than keeps the call inside the M-step kernels' limits - the 1,024
// list entries per UTR of k2_mstep / k3_mstep and the 32-bit offsets of the LDS-DMA kernels (em_choose).
static int em_depth(const std::vector<UtrDesc> &h_desc, int B, const EmSwitches &sw, int n_jobs, int kmax, const int32_t *job_utr,
                    const int32_t *job_fixed) {
    bool any_m = false;
    size_t v1 = 0, pt1 = 0;
    std::vector<int> per_utr(h_desc.size(), 0);
    int max_jobs_utr = 1;
    for (int j = 0; j < n_jobs; ++j) {
        const UtrDesc &d = h_desc[job_utr[j]];
        any_m = any_m || job_fixed[j] == 0;
        v1 += (size_t)d.Np;
        pt1 += (size_t)((d.T * B + MT_ROWS - 1) / MT_ROWS);
        max_jobs_utr = std::max(max_jobs_utr, ++per_utr[job_utr[j]]);
    }
    if (!any_m || em_wide(sw, n_jobs, kmax)) return 1;
    int depth = sw.depth;
    while (depth > 1 && ((size_t)max_jobs_utr * depth > 1024 || v1 * depth * 8 >= ((size_t)1 << 31) || pt1 * depth >= ((size_t)1 << 31)))
        --depth;
    return depth;
}

static int em_choose(const EmPlan &p, const EmSwitches &sw, int n_jobs, int kmax, EmKernels &k) {
    // Small calls (the ~100 jobs of one UTR, or of a few streams' current UTRs) leave most of the GPU idle and an
    // M-step round takes as long as ONE workgroup needs for its pass over a tile: the jobs of a tile are then cut
    // into passes of 16 that separate workgroups take (k2_mstep).  Every score is the same MFMA chain either way,
    // so a UTR's result does not depend on the size of the call it is part of.
    k.wide = em_wide(sw, n_jobs, kmax);
    k.job_split = (long long)p.active.size() * p.tiles_max <= sw.split_maxtiles;
    // k3_mstep unless SCAPE_HIP_MSTEP=v2 asks for k2_mstep (A/B runs; identical bits).  k3's DMA source offsets are
    // 32-bit byte offsets from the start of the job vectors.
    k.ring_mstep = !sw.mstep_v2 && p.vtot * 8 < ((size_t)1 << 31);   // (totals over all column slots)
    // k4_mstep: set-up and epilogue off the critical path - the kernel of wave-sized calls; calls with few live tiles
    // keep k3_mstep with a tile's jobs cut into passes for several workgroups
    k.multi_mstep = k.ring_mstep && !k.job_split && !sw.debug && p.pttot < ((size_t)1 << 31) && !sw.mstep_v3;
    if (k.multi_mstep && M4_LDS_BYTES > 64 * 1024)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k4_mstep), hipFuncAttributeMaxDynamicSharedMemorySize, M4_LDS_BYTES));
    if (k.ring_mstep && M3_LDS_BYTES > 64 * 1024)   // per device; a few microseconds
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k3_mstep), hipFuncAttributeMaxDynamicSharedMemorySize, M3_LDS_BYTES));
    return 0;
}

static int em_upload(scape_hip_ctx *c, const EmPlan &p, size_t nj, int kmax) {
    EmBufs &e = c->batch->em;
    const size_t nc = nj * p.depth;
    if (e.ensure(nj, nc, kmax, c->batch->n_utr, p.vtot, p.pttot)) return 1;
    StreamDrain drain(c->stream);             // the plan's vectors are the caller's: they outlive this wait
    hipStream_t s = c->stream;
    if (to_dev(s, e.elist, p.elist.data(), nj * 4) || (!p.active.empty() && to_dev(s, e.active, p.active.data(), p.active.size() * 4)) ||
        to_dev(s, e.voff, p.voff.data(), nc * 8) || to_dev(s, e.ptoff, p.ptoff.data(), nc * 8) ||
        to_dev(s, e.ujoff, p.ujoff.data(), p.ujoff.size() * 8) || to_dev(s, e.ujlist, p.ujlist.data(), nc * 4))
        return 1;
    return drain.wait();                      // the host vectors are pageable: the copies have left them now
}

// One E-step launch.  The three kernels share their arguments up to the round number, which k2_estep_all_rounds
// (it loops over the rounds itself) does not take.
template <typename Kernel, typename... Round>
static void launch_estep(scape_hip_ctx *c, Kernel kernel, unsigned threads, const EmState &S, int kmax, const int32_t *job_list,
                         int n_jobs, Round... round) {
    const BatchState &b = *c->batch;
    const JobBufs &j = b.job;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(((n_jobs + 7) / 8) * 8)), dim3(threads), 0, c->stream, b.d_desc.as<UtrDesc>(),
                       b.prm, b.d_cnt.as<double>(), b.d_M.as<double>(), kmax, j.utr.as<int32_t>(), j.K.as<int32_t>(),
                       j.fixed.as<int32_t>(), j.a.as<int32_t>(), j.b.as<int32_t>(), j.ws.as<double>(), j.karr.as<int8_t>(), S,
                       j.ao.as<int32_t>(), j.bo.as<int32_t>(), j.wso.as<double>(), j.bic.as<double>(), j.nlb.as<int32_t>(),
                       j.lb.as<double>(), c->d_counters.as<unsigned long long>(), round..., job_list, n_jobs);
}

// The E-step launches of pass r of a call that runs ahead: one per column slot (the last pass only finalises: one).
template <typename Kernel>
static void launch_estep_slots(scape_hip_ctx *c, Kernel kernel, const EmState &S, int kmax, const int32_t *job_list, int n_jobs,
                               int r, int slots, int depth) {
    for (int slot = 0; slot < slots; ++slot) launch_estep(c, kernel, 64, S, kmax, job_list, n_jobs, r, slot, depth);
}

// One M-step launch.  `extent` is the second factor of the grid (tiles, or k4_mstep's tile groups, of the largest UTR);
// `tail` are the two arguments k2_mstep / k3_mstep take beyond k4_mstep's.
template <typename Kernel, typename... Tail>
static void launch_mstep(scape_hip_ctx *c, Kernel kernel, unsigned grid_y, unsigned threads, size_t lds, const EmState &S,
                         int n_active, int extent, Tail... tail) {
    const BatchState &b = *c->batch;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(((n_active + 7) / 8) * 8 * extent), grid_y), dim3(threads), lds, c->stream,
                       b.d_desc.as<UtrDesc>(), b.prm, b.d_M.as<double>(), b.em.active.as<int32_t>(), n_active, extent,
                       b.em.ujoff.as<int64_t>(), b.em.ujlist.as<int32_t>(), S.V, S.Vsuf, S.voff, S.rd_m, S.rd_lo, S.rd_hi,
                       S.rd_lw, S.rd_sv, S.rd_n0, S.rd_n1, S.ptoff, S.pt_score, S.pt_row, b.d_tile_nend.as<int32_t>(),
                       c->d_counters.as<unsigned long long>(), tail...);
}

// SCAPE_HIP_DEBUG: what the M-step of round r did, on stderr
static int em_debug_round(scape_hip_ctx *c, int r, int nround) {
    unsigned long long *dbg = c->batch->em.dbg.as<unsigned long long>();
    if (r < nround) {      // cumulative tensor bytes the M-step has asked for (its own tally), per round
        unsigned long long shard[64], tb = 0;
        HIPCHK(hipMemcpy(shard, c->d_counters.as<unsigned long long>() + CNT_MSTEP_TENSOR, sizeof(shard), hipMemcpyDeviceToHost));
        for (int i = 0; i < 64; ++i) tb += shard[i];
        fprintf(stderr, "[em bytes %d] %llu\n", r, tb);
    }
    if (r == 0 || r == 10 || r == 25 || r == nround - 1) {
        unsigned long long h[24];
        HIPCHK(hipMemcpy(h, dbg, sizeof(h), hipMemcpyDeviceToHost));
        // k3_mstep only: k-steps x jobs if every job stopped at its own support / as run (16-job groups over the union)
        fprintf(stderr, "[em round %d] job-halfchunks own-support %llu, union %llu, padded to groups %llu; sorted-by-n1 groups %llu\n", r, h[16], h[17], h[18], h[19]);
        fprintf(stderr, "[em round %d] tiles %llu active %llu sum_cnt %llu passes %llu | G-hist:", r, h[0], h[1], h[2], h[3]);
        for (int i = 4; i < 16; ++i) fprintf(stderr, " %llu", h[i]);
        fprintf(stderr, "\n");
        HIPCHK(hipMemsetAsync(dbg, 0, 24 * sizeof(unsigned long long), c->stream));
    }
    return 0;
}

// What the launches of a call that runs ahead are sized by: the jobs on the E-step list, the UTRs on the M-step's list,
// the tiles of the largest of those and the slots a pass can still use.  The plan's values until the first shrink.
struct EmLive {
    int jobs, utrs, tiles_max, slots;
};
// One shrink, after the probe of pass r has drained the stream: k_em_shrink compacts both lists on the device, the kept
// UTR list comes back (a second short wait, on the few shrink events of a call only) and the grids follow it.
static int em_shrink(scape_hip_ctx *c, const EmPlan &p, const EmSwitches &sw, int r, std::vector<int32_t> &h_active, EmLive &live) {
    const BatchState &b = *c->batch;
    const EmBufs &em = b.em;
    hipLaunchKernelGGL(k_em_shrink, dim3(1), dim3(EM_SHRINK_THREADS), 0, c->stream, em.elist.as<int32_t>(), live.jobs,
                       em.status.as<int32_t>(), b.job.K.as<int32_t>(), b.job.fixed.as<int32_t>(), em.active.as<int32_t>(), live.utrs,
                       em.udone.as<int32_t>(), em.ujoff.as<int64_t>(), p.depth, em.shrunk.as<int32_t>());
    HIPCHK(hipGetLastError());
    int32_t kept[3] = {0, 0, 0};
    if (to_host(c->stream, kept, em.shrunk, sizeof(kept)) || to_host(c->stream, h_active.data(), em.active, (size_t)live.utrs * 4)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (kept[0] < 1 || kept[0] > live.jobs || kept[1] < 1 || kept[1] > live.utrs) return fail("EM shrink: inconsistent live counts");
    const int slots = em_slots_needed(kept[2], p.depth);
    if (sw.trace)
        fprintf(stderr, "[shrink] pass %d jobs %d -> %d utrs %d -> %d slots %d\n", r, live.jobs, kept[0], live.utrs, kept[1], slots);
    live = EmLive{kept[0], kept[1], em_tiles_max(b.h_desc, b.prm.B, h_active.data(), kept[1]), slots};
    return 0;
}

// the passes of one call: E-step, M-step, ... and a last E-step that finishes the jobs still running.  A job runs up
// to p.depth rounds per pass (one k2_estep launch per slot) and at least one, so nround + 1 passes always do.
static int em_rounds(scape_hip_ctx *c, const EmPlan &p, const EmSwitches &sw, const EmKernels &k, int n_jobs, int kmax) {
    EmBufs &em = c->batch->em;
    // The shrink: late in a call that runs ahead most jobs are finalised and most UTRs have no job left, so the E-step
    // list, the M-step's UTR list and both grids are cut down to what is live (em_shrink).  Placement only: a job's
    // rounds and a column's tiles are the same arithmetic wherever they run.
    const bool shrinking = sw.shrink && p.any_m && !k.wide && !sw.debug;
    const EmState S = em.state(shrinking);
    const int nround = c->batch->prm.nround, n_active = (int)p.active.size(), n_utr = c->batch->n_utr;
    const int32_t *jl = em.elist.as<int32_t>();
    EmLive live{n_jobs, n_active, p.tiles_max, p.depth};
    std::vector<int32_t> h_done, h_active;
    if (shrinking) {
        h_done.assign(n_utr, 0);
        h_active = p.active;
        HIPCHK(hipMemsetAsync(em.udone.p, 0, (size_t)n_utr * 4, c->stream));
    }
    unsigned long long *dbg = nullptr;
    if (sw.debug) {
        if (em.dbg.ensure(24 * sizeof(unsigned long long))) return 1;
        dbg = em.dbg.as<unsigned long long>();
        HIPCHK(hipMemsetAsync(dbg, 0, 24 * sizeof(unsigned long long), c->stream));
    }
    if (!p.any_m) {
        // only fixed-inference jobs (the ws-only re-fits of rm_component): all rounds in one launch (depth 1: columns = jobs)
        if (sw.fine && ev_begin(c, 4)) return 1;
        if (!with_column_class(EstepClasses{}, kmax + 1, [&](auto cm) {
                launch_estep(c, k2_estep_all_rounds<decltype(cm)::value>, 64, S, kmax, em.ujlist.as<int32_t>(), n_jobs);
            }))
            return fail("no E-step kernel for kmax " + std::to_string(kmax));
        HIPCHK(hipGetLastError());
        if (sw.fine && ev_end(c, 4)) return 1;
        return 0;
    }
    // few live tiles: passes of 16 jobs, one workgroup each (gridDim.y covers the longest job list of a UTR)
    const int jobs_per_pass = k.job_split ? 16 : MT_MAXJ;
    const unsigned psplit = k.job_split ? (unsigned)std::min(64, (p.max_cols_utr + 15) / 16) : 1u;
    unsigned long long executed_prev = 0;
    const int probe_mask = (n_jobs >= 8192 && p.depth == 1) ? 7 : 3;
    for (int r = 0; r <= nround; ++r) {
        if (sw.fine && ev_begin(c, 4)) return 1;
        // K up to 63: the column arrays of the 64-column class live in scratch - slow, and rare (a re-run loop that keeps
        // growing, apa_core.py:1023-1030)
        const bool launched =
            k.wide ? with_column_class(WideClasses{}, kmax + 1, [&](auto cm) {
                         launch_estep(c, k2_estep_cs<decltype(cm)::value>, 256, S, kmax, jl, n_jobs, r);
                     })
                   : with_column_class(EstepClasses{}, kmax + 1, [&](auto cm) {
                         launch_estep_slots(c, k2_estep<decltype(cm)::value>, S, kmax, jl, live.jobs, r, r < nround ? live.slots : 1, p.depth);
                     });
        if (!launched) return fail("no E-step kernel for kmax " + std::to_string(kmax));
        HIPCHK(hipGetLastError());
        if (sw.fine && ev_end(c, 4)) return 1;
        if (r < nround) {
            if (sw.fine && ev_begin(c, 5)) return 1;
            if (k.multi_mstep)
                launch_mstep(c, k4_mstep, 1u, 64 * M4_NW, M4_LDS_BYTES, S, live.utrs, (live.tiles_max + M4_TPW - 1) / M4_TPW);
            else if (k.ring_mstep)
                launch_mstep(c, k3_mstep, psplit, 256, M3_LDS_BYTES, S, live.utrs, live.tiles_max, jobs_per_pass, dbg);
            else
                launch_mstep(c, k2_mstep, psplit, 256, 0, S, live.utrs, live.tiles_max, jobs_per_pass, dbg);
            c->h_traffic[3] += 1;
            HIPCHK(hipGetLastError());
            if (sw.fine && ev_end(c, 5)) return 1;
        }
        // early exit: no job executed a round since the last probe -> every job has been finalised.  The probe waits for
        // the stream (a bubble of a few tens of microseconds): every 4 launches for small calls, whose jobs all finish
        // early and whose rounds are short, and for calls that run ahead, which end well before launch nround; every 8
        // for wave-sized ones at one round per launch, which run to the last round anyway
        if (r < nround && (r & probe_mask) == probe_mask) {
            unsigned long long executed = 0, head[CNT_EXEC + 64];     // the counters up to the executed shards: CNT_DONE too
            HIPCHK(hipMemcpyAsync(head, c->d_counters.as<unsigned long long>(), sizeof(head), hipMemcpyDeviceToHost, c->stream));
            if (shrinking && to_host(c->stream, h_done.data(), em.udone, (size_t)n_utr * 4)) return 1;
            HIPCHK(hipStreamSynchronize(c->stream));
            for (int i = 0; i < 64; ++i) executed += head[CNT_EXEC + i];
            if (executed == executed_prev) break;
            executed_prev = executed;
            if (shrinking) {
                const long long live_jobs = (long long)n_jobs - (long long)head[CNT_DONE];
                long long live_utrs = 0;
                for (int i = 0; i < live.utrs; ++i) {
                    const int u = h_active[i];
                    live_utrs += (int64_t)h_done[u] * p.depth < p.ujoff[u + 1] - p.ujoff[u];
                }
                if ((em_shrink_due(live.jobs, live_jobs, sw.shrink_at) || em_shrink_due(live.utrs, live_utrs, sw.shrink_at)) &&
                    em_shrink(c, p, sw, r, h_active, live))
                    return 1;
            }
        }
        if (sw.debug && em_debug_round(c, r, nround)) return 1;
    }
    return 0;
}

// job tables are already on the device
static int em_lockstep(scape_hip_ctx *c, int n_jobs, int kmax, const int32_t *job_utr, const int32_t *job_fixed) {
    const EmSwitches sw = em_switches();
    const BatchState &b = *c->batch;
    const int depth = em_depth(b.h_desc, b.prm.B, sw, n_jobs, kmax, job_utr, job_fixed);
    const EmPlan plan = em_plan(b.h_desc, b.prm.B, (size_t)n_jobs, job_utr, job_fixed, sw.size_order, depth);
    EmKernels kernels;
    if (em_choose(plan, sw, n_jobs, kmax, kernels) || em_upload(c, plan, (size_t)n_jobs, kmax)) return 1;
    return em_rounds(c, plan, sw, kernels, n_jobs, kmax);
}

// ------------------------------------------------------------------------------------------
// host-only halves of the batch entry points: no HIP call, no handle (tools/batch_plan_check.cpp drives them on the CPU)
// ------------------------------------------------------------------------------------------
// The descriptor walk of scape_hip_batch_load: per UTR its offsets into the ragged arrays, the tensors and the tile
// extents, its log-domain bins and whether its theta grid is uniform; over the batch the totals, the maxima and whether
// Phase B may slide.  The arguments are the load's, checked for NULL and the parameter ranges by the caller.
static int batch_plan(const scape_hip_params &p, int n_utr, const int64_t *bin_off, const int64_t *theta_off,
                      const double *all_theta, const double *r, const double *pa, const double *utr_L, const double *min_theta,
                      const double *unif_ll, BatchPlan &out) {
    BatchPlan s;
    double bmax = p.betas[0];
    for (int j = 1; j < p.n_beta; ++j) bmax = std::max(bmax, p.betas[j]);
    s.h_desc.assign(n_utr, UtrDesc());
    bool slide = p.n_beta <= 16;
    for (int u = 0; u < n_utr; ++u) {
        UtrDesc &d = s.h_desc[u];
        const int64_t N = bin_off[u + 1] - bin_off[u], T = theta_off[u + 1] - theta_off[u];
        if (N < 1 || T < 1 || N > (1 << 26) || T > 65535) return fail("UTR " + std::to_string(u) + ": bad n_frag / n_theta");
        const double *th = all_theta + theta_off[u];
        for (int64_t i = 1; i < T; ++i)
            if (!(th[i] >= th[i - 1])) return fail("UTR " + std::to_string(u) + ": all_theta must be ascending");
        d.bin_off = bin_off[u];
        d.theta_off = theta_off[u];
        d.N = (int)N;
        d.Np = round_up((int)N, PITCH);
        d.T = (int)T;
        d.at_off = (int64_t)s.at_total;
        d.m_off = (int64_t)s.m_total;
        d.log_off = (int64_t)s.loglist.size();
        d.tile_off = (int64_t)s.tiles_total;
        const int nt = (int)((T * p.n_beta + TILE_ROWS - 1) / TILE_ROWS);
        s.tiles_total += (size_t)nt;
        s.tiles_max_all = std::max(s.tiles_max_all, nt);
        for (int64_t n = 0; n < N; ++n)
            if (!std::isnan(pa[bin_off[u] + n]) || !std::isnan(r[bin_off[u] + n])) s.loglist.push_back((int32_t)n);
        d.n_log = (int)(s.loglist.size() - (size_t)d.log_off);
        d.mlog_off = (int64_t)s.mlog_total;
        if (d.n_log > 0 && d.n_log <= PB_LOGCAP) s.mlog_total += (size_t)T * p.n_beta * d.n_log;
        s.logbin_utr.insert(s.logbin_utr.end(), (size_t)d.n_log, (int32_t)u);
        // uniform grid of integer values: theta_w - theta_i is exact and depends on w - i only
        d.c_lo = 1;
        d.c_hi = 0;
        const double step0 = (T > 1) ? th[1] - th[0] : 0.0;
        bool uni = step0 > 0.0;
        for (int64_t i = 0; i < T && uni; ++i) uni = std::floor(th[i]) == th[i] && (i == 0 || th[i] - th[i - 1] == step0);
        if (uni) {
            const int rmax = (int)std::floor(3 * bmax / step0) + 1;     // reach of the widest window in grid points, + 1 to spare
            d.c_lo = rmax + 1;
            d.c_hi = (int)T - 2 - rmax;
        }
        if (d.c_lo > d.c_hi) slide = false;
        d.unif_ll = unif_ll[u];
        d.L = utr_L[u];
        d.min_theta = min_theta[u];
        s.at_total += (size_t)T * d.Np;
        s.m_total += (size_t)T * p.n_beta * d.Np;
        s.T_max = std::max(s.T_max, d.T);
        s.Np_max = std::max(s.Np_max, d.Np);
        s.W_max = std::max(s.W_max, max_window(th, d.T, bmax));
    }
    s.n_utr = n_utr;
    s.n_bins = bin_off[n_utr];
    s.n_theta_total = (size_t)theta_off[n_utr];
    s.n_logbins = s.logbin_utr.size();
    s.pb_slide = slide && s.W_max <= 4 * PB_STEPS && s.T_max <= 4096;
    out = std::move(s);
    return 0;
}

// Host-side validation of scape_hip_batch_em's job tables: every index a kernel dereferences is checked here.
static int em_jobs_check(const BatchState &b, int n_jobs, int kmax, const int32_t *job_utr, const int32_t *job_K,
                         const int32_t *job_fixed, const int32_t *alpha_idx, const int32_t *beta_idx, const int8_t *k_arr) {
    const int nround = b.prm.nround, B = b.prm.B;
    for (int j = 0; j < n_jobs; ++j) {
        const int u = job_utr[j], K = job_K[j];
        if (u < 0 || u >= b.n_utr) return fail("job " + std::to_string(j) + ": bad UTR index");
        if (K < 0 || K > kmax) return fail("job " + std::to_string(j) + ": K out of range");
        const int T = b.h_desc[u].T;
        for (int k = 0; k < K; ++k) {
            const int a = alpha_idx[(size_t)j * kmax + k], bi = beta_idx[(size_t)j * kmax + k];
            if (a < 0 || a >= T || bi < 0 || bi >= B) return fail("job " + std::to_string(j) + ": alpha/beta index out of range");
            if (k > 0 && a < alpha_idx[(size_t)j * kmax + k - 1]) return fail("job " + std::to_string(j) + ": alpha indices must be non-decreasing");
        }
        for (int t = 0; t < nround; ++t) {
            const int k = k_arr[(size_t)j * nround + t];
            if (k < 0 || k > K || (K > 0 && k >= K)) return fail("job " + std::to_string(j) + ": k_arr entry out of range");
        }
    }
    // k2_mstep keeps the per-tile list of a UTR's jobs in a fixed LDS table (mstep_staged.inc, s_all)
    std::vector<int32_t> per_utr(b.n_utr, 0);
    for (int j = 0; j < n_jobs; ++j)
        if (!job_fixed[j] && ++per_utr[job_utr[j]] > SCAPE_MAX_JOBS_PER_UTR)
            return fail("UTR " + std::to_string(job_utr[j]) + ": more than " + std::to_string(SCAPE_MAX_JOBS_PER_UTR) +
                        " non-fixed jobs in one call (split the call)");
    return 0;
}

// The same for the model tables of scape_hip_batch_labels.  The output is one label per bin of the batch: two models
// of one UTR in one call would be two workgroups writing the same bins.
static int labels_check(const BatchState &b, int n_sel, int kmax, const int32_t *sel_utr, const int32_t *sel_K,
                        const int32_t *alpha_idx, const int32_t *beta_idx) {
    std::vector<char> named(b.n_utr, 0);
    for (int j = 0; j < n_sel; ++j) {
        const int u = sel_utr[j], K = sel_K[j];
        if (u < 0 || u >= b.n_utr) return fail("labels: bad UTR index");
        if (named[u]) return fail("labels: a UTR is named twice");
        named[u] = 1;
        if (K < 0 || K > kmax) return fail("labels: K out of range");
        for (int k = 0; k < K; ++k) {
            const int a = alpha_idx[(size_t)j * kmax + k], bi = beta_idx[(size_t)j * kmax + k];
            if (a < 0 || a >= b.h_desc[u].T || bi < 0 || bi >= b.prm.B) return fail("labels: alpha/beta index out of range");
        }
    }
    return 0;
}

static void report_release(scape_hip_ctx *c);   // report.inc

extern "C" {

int scape_hip_abi_version(void) { return SCAPE_HIP_ABI_VERSION; }
const char *scape_hip_last_error(void) { return g_err.c_str(); }

int scape_hip_device_count(int *count) {
    if (!count) return fail("count is NULL");
    HIPCHK(hipGetDeviceCount(count));
    return 0;
}

int scape_hip_create(int device, scape_hip_ctx **out) {
    if (!out) return fail("out is NULL");
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail("no such HIP device: " + std::to_string(device));
    HIPCHK(hipSetDevice(device));
    scape_hip_ctx *c = new scape_hip_ctx();
    c->device = device;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    snprintf(c->name, sizeof(c->name), "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    HIPCHK(hipStreamCreate(&c->stream));
    if (c->d_counters.ensure(N_COUNTERS * sizeof(unsigned long long))) return 1;
    *out = c;
    return 0;
}

int scape_hip_device_name(scape_hip_ctx *c, char *buf, int buflen) {
    if (!c || !buf || buflen <= 0) return fail("bad argument");
    snprintf(buf, buflen, "%s", c->name);
    return 0;
}

int scape_hip_batch_free(scape_hip_ctx *c) {
    CTX_ENTER(c);
    c->batch.reset();   // every DevBuf of the batch frees itself, and none of its scalars outlives it
    return 0;
}

// The handle's device memory goes while the device is current and before the stream is destroyed: the batch and the
// report state each as one, the handle's own two buffers here, so that `delete c` finds nothing left to free.
int scape_hip_destroy(scape_hip_ctx *c) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->batch.reset();
    report_release(c);
    c->d_err.release();
    c->d_counters.release();
    for (int w = 0; w < 6; ++w)
        for (auto &e : c->ev[w]) {
            (void)hipEventDestroy(e.a);
            (void)hipEventDestroy(e.b);
        }
    (void)hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

// ---- operator level ------------------------------------------------------------------------
// The frame of an operator call: its device arrays, which free themselves on every return, and the drain that waits
// ahead of that for whatever the call has queued on the caller's arrays.
struct OpCall {
    DevBuf in[3], out;
    StreamDrain drain;
    explicit OpCall(scape_hip_ctx *c) : drain(c->stream, false) {}
    double *dev(int i) const { return in[i].as<double>(); }
};
static int op_common(scape_hip_ctx *c, int n, const double *const *in, int n_in, OpCall &k) {
    if (n < 0) return fail("negative length");
    if (set_device(c)) return 1;
    const size_t bytes = (size_t)n * sizeof(double);
    for (int i = 0; i < n_in; ++i) {
        if (!in[i] && n > 0) return fail("NULL input array");
        if (k.in[i].ensure(std::max<size_t>(16, bytes))) return 1;
        k.drain.armed = true;
        if (n) HIPCHK(hipMemcpyAsync(k.in[i].p, in[i], bytes, hipMemcpyHostToDevice, c->stream));
    }
    return k.out.ensure(std::max<size_t>(16, bytes));
}
static int op_finish(scape_hip_ctx *c, int n, OpCall &k, double *out) {
    HIPCHK(hipGetLastError());
    if (n) HIPCHK(hipMemcpyAsync(out, k.out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return k.drain.wait();
}

int scape_hip_loglik_xlr_t_pa(scape_hip_ctx *c, const double *x, const double *l, const double *pa,
                              int32_t n, double theta, double sigma_f, double *out) {
    CTX_GUARD(c);
    const double *in[3] = {x, l, pa};
    OpCall k(c);
    if (op_common(c, n, in, 3, k)) return 1;
    if (n) hipLaunchKernelGGL(k_op_pa, dim3((n + 255) / 256), dim3(256), 0, c->stream, k.dev(0), k.dev(1), k.dev(2), n, theta, sigma_f, k.out.as<double>());
    return op_finish(c, n, k, out);
}

int scape_hip_loglik_xlr_t_r_known(scape_hip_ctx *c, const double *x, const double *l, const double *r,
                                   int32_t n, const double *s_dis, const double *pmf_s, int32_t n_s,
                                   double theta, double mu_f, double sigma_f, double *out) {
    CTX_GUARD(c);
    if (n_s < 1 || n_s > SCAPE_MAX_S) return fail("n_s out of range");
    DevParams P;
    fill_params(P, mu_f, sigma_f, 0, 0, nullptr, n_s, s_dis, pmf_s, 0);
    const double *in[3] = {x, l, r};
    OpCall k(c);
    if (op_common(c, n, in, 3, k)) return 1;
    if (n) hipLaunchKernelGGL(k_op_r_known, dim3((n + 255) / 256), dim3(256), 0, c->stream, k.dev(0), k.dev(1), k.dev(2), n, P, theta, k.out.as<double>());
    return op_finish(c, n, k, out);
}

int scape_hip_loglik_xlr_t_r_unknown(scape_hip_ctx *c, const double *x, const double *l, const double *r,
                                     int32_t n, const double *s_dis, const double *pmf_s, int32_t n_s,
                                     double theta, double mu_f, double sigma_f, double *out) {
    CTX_GUARD(c);
    (void)r;
    if (n_s < 1 || n_s > SCAPE_MAX_S) return fail("n_s out of range");
    DevParams P;
    fill_params(P, mu_f, sigma_f, 0, 0, nullptr, n_s, s_dis, pmf_s, 0);
    const double *in[2] = {x, l};
    OpCall k(c);
    if (op_common(c, n, in, 2, k)) return 1;
    if (n) hipLaunchKernelGGL(k_op_r_unknown, dim3((n + 255) / 256), dim3(256), 0, c->stream, k.dev(0), k.dev(1), n, P, theta, k.out.as<double>());
    return op_finish(c, n, k, out);
}

int scape_hip_get_loglik_marginal_tensor(scape_hip_ctx *c, const double *all_theta, int32_t T,
                                         const double *betas, int32_t B, const double *A, int32_t N,
                                         double *out) {
    if (!c) return fail("ctx is NULL");
    if (T < 1 || N < 1) return fail("empty theta grid or no fragments");
    if (B < 1 || B > SCAPE_MAX_BETA) return fail("n_beta out of range");
    if (!all_theta || !betas || !A || !out) return fail("NULL argument");
    CTX_ENTER(c);
    if (finish_build(c)) return 1;   // this call reuses the handle's error word: read a queued build's flag first
    for (int i = 1; i < T; ++i)
        if (!(all_theta[i] >= all_theta[i - 1])) return fail("all_theta must be ascending");
    DevParams P;
    fill_params(P, 0, 1, 0, B, betas, 0, nullptr, nullptr, 0);
    const int Np = round_up(N, PITCH);
    double bmax = betas[0];
    for (int j = 1; j < B; ++j) bmax = std::max(bmax, betas[j]);
    const int Wmax = max_window(all_theta, T, bmax);
    std::vector<double> at((size_t)T * Np, 0.0);
    for (int n = 0; n < N; ++n)
        for (int t = 0; t < T; ++t) at[(size_t)t * Np + n] = A[(size_t)n * T + t];
    PhaseB ch;
    if (phase_b_choose(B, Wmax, T, false, "v2", ch)) return 1;   // form 0, whatever the environment asks of a batch
    BatchState t;   // one UTR of log-domain bins only, on buffers of the call's own: they free themselves with it
    t.prm = P;
    t.n_utr = 1;
    t.T_max = T;
    t.h_desc.assign(1, UtrDesc());
    t.h_desc[0].N = N;
    t.h_desc[0].Np = Np;
    t.h_desc[0].T = T;
    if (t.d_AT.ensure(at.size() * sizeof(double)) || t.d_M.ensure((size_t)T * B * Np * sizeof(double)) ||
        t.d_theta.ensure((size_t)T * sizeof(double)) || t.d_desc.ensure(sizeof(UtrDesc)))
        return 1;
    StreamDrain drain(c->stream);   // `at` and `t` stand ahead of it
    if (to_dev(c->stream, t.d_AT, at.data(), at.size() * sizeof(double)) || to_dev(c->stream, t.d_theta, all_theta, (size_t)T * sizeof(double)) ||
        to_dev(c->stream, t.d_desc, t.h_desc.data(), sizeof(UtrDesc)) || queue_phase_b(c, t, ch, 1) ||
        check_err_flag(c, "get_loglik_marginal_tensor"))
        return 1;
    HIPCHK(hipMemcpy2DAsync(out, (size_t)N * sizeof(double), t.d_M.p, (size_t)Np * sizeof(double), (size_t)N * sizeof(double),
                            (size_t)T * B, hipMemcpyDeviceToHost, c->stream));
    return drain.wait();
}

// ---- batched level ---------------------------------------------------------------------------
int scape_hip_batch_load(scape_hip_ctx *c, const scape_hip_params *p, int32_t n_utr, const int64_t *bin_off,
                         const double *x, const double *l, const double *r, const double *pa,
                         const double *cnt, const int64_t *theta_off, const double *all_theta,
                         const double *utr_L, const double *min_theta, const double *unif_ll) {
    if (!c || !p) return fail("NULL ctx/params");
    if (n_utr < 1 || n_utr > 65535) return fail("n_utr must be in [1, 65535] per batch");
    if (p->n_beta < 1 || p->n_beta > SCAPE_MAX_BETA) return fail("n_beta out of range");
    if (p->n_s < 1 || p->n_s > SCAPE_MAX_S) return fail("n_s out of range");
    if (p->nround < 1 || p->nround > 127) return fail("nround out of range");
    if (!bin_off || !x || !l || !r || !pa || !cnt || !theta_off || !all_theta || !utr_L || !min_theta || !unif_ll)
        return fail("NULL array argument");
    CTX_ENTER(c);
    HIPCHK(hipStreamSynchronize(c->stream));   // a queued build of the previous batch still reads its buffers
    if (!c->batch) c->batch.reset(new BatchState());   // a loaded handle keeps its state: the buffers are reused
    BatchState &b = *c->batch;
    b.loaded = b.built = b.build_unchecked = false;   // a load refused below leaves the handle unloaded
    BatchPlan plan;
    if (batch_plan(*p, n_utr, bin_off, theta_off, all_theta, r, pa, utr_L, min_theta, unif_ll, plan)) return 1;
    fill_params(b.prm, p->mu_f, p->sigma_f, p->max_unif_ws, p->n_beta, p->betas, p->n_s, p->s_dis, p->pmf_s, p->nround);
    static_cast<BatchShape &>(b) = std::move(plan);   // the lists stay in `plan` for the upload
    const std::vector<int32_t> &loglist = plan.loglist, &logbin_utr = plan.logbin_utr;
    const int64_t nb = b.n_bins, nt = (int64_t)b.n_theta_total;

    const bool trace_load = getenv("SCAPE_HIP_DEBUG") != nullptr;
    const auto t_alloc0 = std::chrono::steady_clock::now();
    hipStream_t s = c->stream;
    StreamDrain drain(s);   // `plan` and the descriptors stand ahead of it
    if (b.d_x.ensure(nb * 8) || b.d_l.ensure(nb * 8) || b.d_r.ensure(nb * 8) || b.d_pa.ensure(nb * 8) ||
        b.d_cnt.ensure(nb * 8) || b.d_theta.ensure(nt * 8) || b.d_desc.ensure(n_utr * sizeof(UtrDesc)) ||
        b.d_loglist.ensure(loglist.size() * 4) || b.d_AT.ensure(b.at_total * 8) || b.d_V.ensure(b.at_total * 8) ||
        b.d_M.ensure(b.m_total * 8) || b.d_tile_nend.ensure(b.tiles_total * 4))
        return 1;
    if (p->n_beta <= 16) {   // the three-kernel Phase B (phase_b.inc)
        const size_t WP = (size_t)(((b.W_max + 3) & ~3) + 1);
        if (b.d_tbi.ensure((size_t)nt * 40 * 4) || b.d_tbG.ensure((size_t)nt * 16 * 8) || b.d_tbpm.ensure((size_t)nt * 16 * WP * 8) ||
            b.d_mlog.ensure(b.mlog_total * 8) || b.d_logbin.ensure(logbin_utr.size() * 4) ||
            (!logbin_utr.empty() && to_dev(s, b.d_logbin, logbin_utr.data(), logbin_utr.size() * 4)))
            return 1;
    }
    const auto t_up0 = std::chrono::steady_clock::now();
    if (to_dev(s, b.d_x, x, nb * 8) || to_dev(s, b.d_l, l, nb * 8) || to_dev(s, b.d_r, r, nb * 8) || to_dev(s, b.d_pa, pa, nb * 8) ||
        to_dev(s, b.d_cnt, cnt, nb * 8) || to_dev(s, b.d_theta, all_theta, nt * 8) ||
        to_dev(s, b.d_desc, b.h_desc.data(), n_utr * sizeof(UtrDesc)) ||
        (!loglist.empty() && to_dev(s, b.d_loglist, loglist.data(), loglist.size() * 4)))
        return 1;
    if (drain.wait()) return 1;
    if (trace_load) {
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "scape_hip_batch_load: %d UTRs, tensors %.2f GB, device buffers (re)allocated in %.1f ms, uploads %.1f ms\n", n_utr,
                (double)(b.m_total + 2 * b.at_total) * 8e-9, std::chrono::duration<double, std::milli>(t_up0 - t_alloc0).count(),
                std::chrono::duration<double, std::milli>(t1 - t_up0).count());
    }
    b.loaded = true;
    return 0;
}

int scape_hip_batch_bytes(scape_hip_ctx *c, int64_t *bytes_batch, int64_t *bytes_free, int64_t *bytes_total) {
    CTX_ENTER(c);
    size_t f = 0, t = 0;
    HIPCHK(hipMemGetInfo(&f, &t));
    const BatchState *b = c->batch.get();
    // (+ the column vectors and per-tile partials of the batch's EM calls so far: EM_DEPTH slots per job, EmBufs)
    if (bytes_batch)
        *bytes_batch = b && b->loaded ? (int64_t)((2 * b->at_total + b->m_total) * 8 + b->n_bins * 40 + b->em.V.cap + b->em.Vsuf.cap +
                                                  b->em.pt_score.cap + b->em.pt_row.cap)
                                      : 0;
    if (bytes_free) *bytes_free = (int64_t)f;
    if (bytes_total) *bytes_total = (int64_t)t;
    return 0;
}

int scape_hip_batch_phase_b_form(scape_hip_ctx *c, int32_t *form) {
    if (!c || !form) return fail("ctx / form is NULL");
    BUILT_BATCH(c, b);
    *form = b.pb_form;
    return 0;
}

int scape_hip_batch_build(scape_hip_ctx *c) {
    CTX_GUARD(c);
    if (!c->batch || !c->batch->loaded) return fail("no batch loaded");
    BatchState &b = *c->batch;
    if (set_device(c) || finish_build(c)) return 1;   // a second build on the handle must not wipe the first one's pending flag
    PhaseB pb;                       // the environment is read at every build; a refusal leaves nothing queued
    if (phase_b_choose(b.prm.B, b.W_max, b.T_max, b.pb_slide, getenv("SCAPE_HIP_PHASE_B"), pb)) return 1;
    dim3 grid((b.Np_max + 255) / 256, (b.T_max + PA_TT - 1) / PA_TT, b.n_utr);
    if (ev_begin(c, 0)) return 1;
    hipLaunchKernelGGL(k_phase_a, grid, dim3(256), 0, c->stream, b.d_desc.as<UtrDesc>(), b.prm, b.d_x.as<double>(),
                       b.d_l.as<double>(), b.d_r.as<double>(), b.d_pa.as<double>(), b.d_theta.as<double>(),
                       b.d_AT.as<double>(), b.d_V.as<double>());
    HIPCHK(hipGetLastError());
    if (ev_end(c, 0) || ev_begin(c, 1)) return 1;
    HIPCHK(hipMemsetAsync(b.d_tile_nend.p, 0, b.tiles_total * 4, c->stream));   // Phase B raises the extents by atomicMax
    b.pb_form = pb.form;
    if (queue_phase_b(c, b, pb) || ev_end(c, 1)) return 1;
    // The kernels are only queued here: the caller's next call (normally scape_hip_batch_em, whose host-side table
    // checks then run while the GPU builds the tensors) launches behind them on the same stream, and reads the
    // consistency flag at its own synchronisation point.  SCAPE_HIP_SYNC_BUILD restores the synchronous behaviour.
    b.build_unchecked = true;
    b.built = true;
    if (getenv("SCAPE_HIP_SYNC_BUILD") && finish_build(c)) return 1;
    return 0;
}

int scape_hip_batch_em(scape_hip_ctx *c, int32_t n_jobs, int32_t kmax, const int32_t *job_utr,
                       const int32_t *job_K, const int32_t *job_fixed, const int32_t *alpha_idx,
                       const int32_t *beta_idx, const double *ws, const int8_t *k_arr,
                       int32_t *alpha_idx_out, int32_t *beta_idx_out, double *ws_out, double *bic_out,
                       int32_t *n_lb_out, double *lb_out) {
    BUILT_BATCH(c, b);
    if (n_jobs < 1) return fail("n_jobs < 1");
    if (kmax < 1 || kmax > SCAPE_MAX_K) return fail("kmax out of range");
    if (!job_utr || !job_K || !job_fixed || !alpha_idx || !beta_idx || !ws || !k_arr || !alpha_idx_out ||
        !beta_idx_out || !ws_out || !bic_out || !n_lb_out)
        return fail("NULL array argument");          // lb_out may be NULL: scape_hip_batch_em_fetch_lb
    if (set_device(c)) return 1;
    b.last_em_jobs = 0;
    if (em_jobs_check(b, n_jobs, kmax, job_utr, job_K, job_fixed, alpha_idx, beta_idx, k_arr)) return 1;
    JobBufs &j = b.job;
    hipStream_t s = c->stream;
    const size_t nj = n_jobs, i4 = nj * 4, k4 = nj * kmax * 4, w8 = nj * (kmax + 1) * 8, ka = nj * b.prm.nround, lb8 = ka * 8;
    if (j.utr.ensure(i4) || j.K.ensure(i4) || j.fixed.ensure(i4) || j.a.ensure(k4) || j.b.ensure(k4) || j.ws.ensure(w8) ||
        j.karr.ensure(ka) || j.ao.ensure(k4) || j.bo.ensure(k4) || j.wso.ensure(w8) || j.bic.ensure(nj * 8) || j.nlb.ensure(i4) ||
        j.lb.ensure(lb8))
        return 1;
    unsigned long long hc[N_COUNTERS];
    StreamDrain drain(s);   // from here on the caller's arrays and `hc` have copies queued on them
    if (to_dev(s, j.utr, job_utr, i4) || to_dev(s, j.K, job_K, i4) || to_dev(s, j.fixed, job_fixed, i4) || to_dev(s, j.a, alpha_idx, k4) ||
        to_dev(s, j.b, beta_idx, k4) || to_dev(s, j.ws, ws, w8) || to_dev(s, j.karr, k_arr, ka))
        return 1;
    HIPCHK(hipMemsetAsync(c->d_counters.p, 0, N_COUNTERS * sizeof(unsigned long long), s));
    HIPCHK(hipMemsetAsync(j.lb.p, 0, lb8, s));
    c->h_traffic[3] = 0;
    if (ev_begin(c, 2) || em_lockstep(c, n_jobs, kmax, job_utr, job_fixed) || ev_end(c, 2)) return 1;
    if (to_host(s, alpha_idx_out, j.ao, k4) || to_host(s, beta_idx_out, j.bo, k4) || to_host(s, ws_out, j.wso, w8) ||
        to_host(s, bic_out, j.bic, nj * 8) || to_host(s, n_lb_out, j.nlb, i4) || (lb_out && to_host(s, lb_out, j.lb, lb8)) ||
        to_host(s, hc, c->d_counters, sizeof(hc)))
        return 1;
    if (drain.wait()) return 1;
    if (finish_build(c)) return 1;        // a batch_build queued before this call: its flag is final now
    b.last_em_jobs = n_jobs;
#ifdef M4_STAMPS   // tools-only: k4_mstep's half-chunk iterations by running column groups and wavefront role (whole call)
    {
        const unsigned long long *st = hc + 4 + 5 * 64 + 16;
        for (int ga = 0; ga < 4; ++ga)
            for (int role = 0; role < 2; ++role) {
                const double n = (double)st[32 + ga * 2 + role];
                const unsigned long long *v = st + 4 * (ga * 2 + role);
                if (n > 0)
                    fprintf(stderr, "[mstep stamps] %d running groups, %s wavefronts: %.3g iterations; mean cycles: dma wait %.0f, barrier %.0f, issue %.0f, reads+mfma %.0f (total %.0f)\n",
                            ga + 1, role ? "vector" : "tile", n, v[0] / n, v[1] / n, v[2] / n, v[3] / n, (v[0] + v[1] + v[2] + v[3]) / n);
            }
    }
#endif
#ifdef ESTEP_STAMPS   // tools-only: where a k2_estep wavefront's lifetime goes (cycle sums over all job-rounds of the call)
    {
        const unsigned long long *st = hc + 4 + 5 * 64;
        const double n = (double)st[7];
        if (n > 0)
            fprintf(stderr, "[estep stamps] job-rounds %.0f; mean cycles: set-up %.0f, bin loop %.0f, reductions+weights %.0f, suffix sums %.0f, tail %.0f (total %.0f)\n",
                    n, st[0] / n, st[1] / n, st[2] / n, st[3] / n, st[4] / n, (st[0] + st[1] + st[2] + st[3] + st[4]) / n);
    }
#endif
    for (int i = 0; i < 3; ++i) c->h_counters[i] = hc[i];
    c->h_traffic[0] = c->h_traffic[1] = c->h_traffic[2] = 0;
    for (int i = 0; i < 64; ++i) {
        c->h_counters[1] += hc[CNT_SLAB + i];   // sharded slab-element counter of the lock-step EM
        c->h_traffic[0] += hc[CNT_MSTEP_TENSOR + i];
        c->h_traffic[1] += hc[CNT_MSTEP_VREQ + i];
        c->h_traffic[2] += hc[CNT_MSTEP_VUNI + i];
    }
    return 0;
}

__global__ void k_gather_rows(const double *__restrict__ src, const int32_t *__restrict__ idx, double *__restrict__ dst,
                              int rowlen, int n_sel) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_sel * rowlen) dst[i] = src[(size_t)idx[i / rowlen] * rowlen + i % rowlen];
}

int scape_hip_batch_em_fetch_lb(scape_hip_ctx *c, int32_t n_sel, const int32_t *job_idx, double *lb_out) {
    if (!c) return fail("ctx is NULL");
    if (n_sel < 1 || !job_idx || !lb_out) return fail("fetch_lb: bad arguments");
    CTX_ENTER(c);
    if (finish_build(c)) return 1;
    BatchState *b = c->batch.get();
    if (!b || b->last_em_jobs < 1) return fail("fetch_lb: no completed scape_hip_batch_em call on this handle");
    for (int i = 0; i < n_sel; ++i)
        if (job_idx[i] < 0 || job_idx[i] >= b->last_em_jobs) return fail("fetch_lb: job index out of range");
    const int nround = b->prm.nround;
    JobBufs &j = b->job;
    if (j.sel.ensure((size_t)n_sel * 4) || j.lbsel.ensure((size_t)n_sel * nround * 8)) return 1;
    StreamDrain drain(c->stream);
    if (to_dev(c->stream, j.sel, job_idx, (size_t)n_sel * 4)) return 1;
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((n_sel * nround + 255) / 256)), dim3(256), 0, c->stream,
                       j.lb.as<double>(), j.sel.as<int32_t>(), j.lbsel.as<double>(), nround, n_sel);
    HIPCHK(hipGetLastError());
    return to_host(c->stream, lb_out, j.lbsel, (size_t)n_sel * nround * 8) || drain.wait();
}

int scape_hip_batch_labels(scape_hip_ctx *c, int32_t n_sel, int32_t kmax, const int32_t *sel_utr,
                           const int32_t *sel_K, const int32_t *alpha_idx, const int32_t *beta_idx,
                           const double *ws, int32_t *labels_out) {
    BUILT_BATCH(c, b);
    if (n_sel < 1) return fail("n_sel < 1");
    if (kmax < 1 || kmax > SCAPE_MAX_K) return fail("kmax out of range");
    if (!sel_utr || !sel_K || !alpha_idx || !beta_idx || !ws || !labels_out) return fail("NULL array argument");
    if (set_device(c)) return 1;
    if (labels_check(b, n_sel, kmax, sel_utr, sel_K, alpha_idx, beta_idx)) return 1;
    LabelBufs &lab = b.lab;
    hipStream_t s = c->stream;
    const size_t ns = n_sel, i4 = ns * 4, k4 = ns * kmax * 4, w8 = ns * (kmax + 1) * 8;
    if (lab.utr.ensure(i4) || lab.K.ensure(i4) || lab.a.ensure(k4) || lab.b.ensure(k4) || lab.ws.ensure(w8) ||
        lab.labels.ensure((size_t)b.n_bins * 4))
        return 1;
    StreamDrain drain(s);
    if (to_dev(s, lab.utr, sel_utr, i4) || to_dev(s, lab.K, sel_K, i4) || to_dev(s, lab.a, alpha_idx, k4) ||
        to_dev(s, lab.b, beta_idx, k4) || to_dev(s, lab.ws, ws, w8) || ev_begin(c, 3))
        return 1;
    if (!with_column_class(LabelClasses{}, kmax + 1, [&](auto cm) {
            hipLaunchKernelGGL(k_labels<decltype(cm)::value>, dim3(n_sel), dim3(256), 0, c->stream, b.d_desc.as<UtrDesc>(), b.prm,
                               b.d_cnt.as<double>(), b.d_M.as<double>(), kmax, lab.utr.as<int32_t>(), lab.K.as<int32_t>(),
                               lab.a.as<int32_t>(), lab.b.as<int32_t>(), lab.ws.as<double>(), lab.labels.as<int32_t>());
        }))
        return fail("no label kernel for kmax " + std::to_string(kmax));
    HIPCHK(hipGetLastError());
    if (ev_end(c, 3)) return 1;
    // copy back only the selected UTRs' bins; contiguous runs of selected UTRs go in one transfer
    std::vector<char> sel(b.n_utr, 0);
    for (int j = 0; j < n_sel; ++j) sel[sel_utr[j]] = 1;
    for (int u = 0; u < b.n_utr; ++u) {
        if (!sel[u]) continue;
        int v = u;
        while (v + 1 < b.n_utr && sel[v + 1]) ++v;
        const int64_t b0 = b.h_desc[u].bin_off, b1 = b.h_desc[v].bin_off + b.h_desc[v].N;
        HIPCHK(hipMemcpyAsync(labels_out + b0, lab.labels.as<int32_t>() + b0, (size_t)(b1 - b0) * 4, hipMemcpyDeviceToHost, s));
        u = v;
    }
    if (drain.wait()) return 1;
    return finish_build(c);
}

int scape_hip_batch_fetch_loglik(scape_hip_ctx *c, int32_t utr, double *A_out) {
    if (!c || !A_out) return fail("NULL argument");
    BUILT_BATCH(c, b);
    if (utr < 0 || utr >= b.n_utr) return fail("bad UTR index");
    if (set_device(c) || finish_build(c)) return 1;
    const UtrDesc &d = b.h_desc[utr];
    std::vector<double> at((size_t)d.T * d.Np);
    HIPCHK(hipMemcpy(at.data(), b.d_AT.as<double>() + d.at_off, at.size() * 8, hipMemcpyDeviceToHost));
    for (int n = 0; n < d.N; ++n)
        for (int t = 0; t < d.T; ++t) A_out[(size_t)n * d.T + t] = at[(size_t)t * d.Np + n];
    return 0;
}

int scape_hip_batch_fetch_tensor(scape_hip_ctx *c, int32_t utr, double *M_out) {
    if (!c || !M_out) return fail("NULL argument");
    BUILT_BATCH(c, b);
    if (utr < 0 || utr >= b.n_utr) return fail("bad UTR index");
    if (set_device(c) || finish_build(c)) return 1;
    const UtrDesc &d = b.h_desc[utr];
    HIPCHK(hipMemcpy2D(M_out, (size_t)d.N * 8, b.d_M.as<double>() + d.m_off, (size_t)d.Np * 8, (size_t)d.N * 8,
                       (size_t)d.T * b.prm.B, hipMemcpyDeviceToHost));
    return 0;
}

int scape_hip_timing_reset(scape_hip_ctx *c) {
    CTX_ENTER(c);
    if (ev_collect(c)) return 1;
    for (int w = 0; w < 6; ++w) {
        c->ms_acc[w] = 0;
        c->n_acc[w] = 0;
    }
    return 0;
}

int scape_hip_timing_get(scape_hip_ctx *c, int32_t which, double *ms_total, int32_t *n_launches) {
    if (which < 0 || which > 5) return fail("which out of range");
    CTX_ENTER(c);
    if (ev_collect(c)) return 1;
    if (ms_total) *ms_total = c->ms_acc[which];
    if (n_launches) *n_launches = c->n_acc[which];
    return 0;
}

int scape_hip_em_counters(scape_hip_ctx *c, int64_t *rounds, int64_t *slab_elems, int64_t *z_elems) {
    if (!c) return fail("ctx is NULL");
    if (rounds) *rounds = (int64_t)c->h_counters[0];
    if (slab_elems) *slab_elems = (int64_t)c->h_counters[1];
    if (z_elems) *z_elems = (int64_t)c->h_counters[2];
    return 0;
}

int scape_hip_em_traffic(scape_hip_ctx *c, int64_t *mstep_tensor_bytes, int64_t *mstep_v_bytes_requested,
                         int64_t *mstep_v_bytes_unique, int64_t *mstep_launches) {
    if (!c) return fail("ctx is NULL");
    if (mstep_tensor_bytes) *mstep_tensor_bytes = (int64_t)c->h_traffic[0];
    if (mstep_v_bytes_requested) *mstep_v_bytes_requested = (int64_t)c->h_traffic[1];
    if (mstep_v_bytes_unique) *mstep_v_bytes_unique = (int64_t)c->h_traffic[2];
    if (mstep_launches) *mstep_launches = (int64_t)c->h_traffic[3];
    return 0;
}

}  // extern "C"

#include "report.inc"
#include "report_mtx.inc"
#include "perm.inc"
