// L-BFGS on the device (pinn_lbfgs_* of include/pinn_hip.h): the optimizer of the reference's committed entry points (INF:122-129,321-335;
// PLATE:220-247,508-559) as three launches per evaluation, whatever the history length:
//   dots_kernel    one bandwidth pass over the held history rows: every inner product the update needs, per-block fp64 partials
//   solve_kernel   ONE workgroup: fixed-order second stage of the reduction, the loss  sum_j c_j sums[j], the scalar state machine (strong-Wolfe line
//                  search after More-Thuente's dcsrch / dcstep, scipy's stop rules, curvature skip), the m x m products' new row / column and the
//                  two triangular solves of the compact representation (Byrd-Nocedal-Schnabel) in fp64 out of LDS
//   update_kernel  one pass: store the new pair, move x_k / g_k, form d = -(gamma g + S a + gamma Y b), write the next trial point
// No atomics, no cross-workgroup waiting: order comes from the stream, results are a deterministic function of the inputs.
// Everything lives in one caller-owned state buffer (make_layout); the library keeps nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pinn {
namespace lbfgs {

constexpr int MAX_M = 64;          // history pairs
constexpr int MAX_SUMS = 128;      // loss sums the coefficient vector covers (5 slots x 16 of the 3-D class is the largest user: 80)
constexpr int RING = 1024;         // per-evaluation losses kept
constexpr int GRID = 256;          // workgroups of the two vector passes (one per compute unit); the dots pass uses the first `gactive`
constexpr int NSCAL = 8;
constexpr int QMAX = 4 * MAX_M + NSCAL;      // quantities per block: (S_j.g, S_j.y, Y_j.g, Y_j.y) per slot, then the scalars
enum { Q_SY = 0, Q_YY, Q_SG, Q_YG, Q_GG, Q_GD, Q_GMAX, Q_BAD };      // scalars: s.y, y.y, s.g, y.g, g.g, g.d, max|g|, non-finite entries of g

enum { ST_RUNNING = 0, ST_GTOL = 1, ST_FTOL = 2, ST_MAXITER = 3, ST_MAXFUN = 4, ST_LINESEARCH = 5, ST_NONFINITE_START = 6, ST_NONFINITE_GRAD = 7 };
enum { ACT_NONE = 0, ACT_TRIAL = 1, ACT_ACCEPT = 2, ACT_INIT = 3, ACT_RESTART = 4 };

struct Record {                    // == pinn_lbfgs_record (what pinn_lbfgs_status copies out)
    int status, iterations, evaluations, pairs, skipped, trials;
    long long loss_pos;
    double f, gmax, step;
};

struct Header {
    Record rec;
    long long P;
    int m, n_sums, maxiter, maxfun, maxls, gactive, chunk, phase, head, action, slot, restarted;
    float grad_scale;
    int pad_;
    double ftol, gtol;
    double alpha, gamma, gg;
    // line search (dcsrch's save area)
    double stx, fx, gx, sty, fy, gy, finit, ginit, gtest, width, width1, stmin, stmax;
    int brackt, stage, ynan, pad2_;
    double coeff[MAX_SUMS];
    double p[MAX_M], q[MAX_M], a[MAX_M], b[MAX_M];      // S^T g, Y^T g at x_k; the coefficients of the direction (by ring slot)
};

struct Layout {
    size_t sy, yy, ring, part, x, g, d, S, Y, total;
    long stride;
};

__host__ __device__ inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

__host__ __device__ inline Layout make_layout(long long P, int m) {
    Layout L;
    L.stride = (long)((P + 3) & ~3LL);                   // rows start 16-byte aligned
    size_t o = up256(sizeof(Header));
    L.sy = o;   o += (size_t)MAX_M * MAX_M * 8;
    L.yy = o;   o += (size_t)MAX_M * MAX_M * 8;
    L.ring = o; o += (size_t)RING * 8;
    L.part = o; o += (size_t)GRID * QMAX * 8;
    const size_t vec = up256((size_t)L.stride * 4);
    L.x = o; o += vec;
    L.g = o; o += vec;
    L.d = o; o += vec;
    L.S = o; o += up256((size_t)m * L.stride * 4);
    L.Y = o; o += up256((size_t)m * L.stride * 4);
    L.total = o;
    return L;
}

struct InitArgs {
    long long P;
    int m, n_sums, maxiter, maxfun, maxls;
    float grad_scale;
    double ftol, gtol;
    float coeff[MAX_SUMS];
};

typedef float lb_f4 __attribute__((ext_vector_type(4)));

template <int W> __device__ __forceinline__ void ld(const float* p, float* out);
template <> __device__ __forceinline__ void ld<1>(const float* p, float* out) { out[0] = *p; }
template <> __device__ __forceinline__ void ld<4>(const float* p, float* out) {
    const lb_f4 v = *reinterpret_cast<const lb_f4*>(p);
    out[0] = v[0]; out[1] = v[1]; out[2] = v[2]; out[3] = v[3];
}
template <int W> __device__ __forceinline__ void st(float* p, const float* in);
template <> __device__ __forceinline__ void st<1>(float* p, const float* in) { *p = in[0]; }
template <> __device__ __forceinline__ void st<4>(float* p, const float* in) {
    lb_f4 v;
    v[0] = in[0]; v[1] = in[1]; v[2] = in[2]; v[3] = in[3];
    *reinterpret_cast<lb_f4*>(p) = v;
}

// The optimizer's gradient element gn = grad_scale * grad and the pair element y = gn - g_k, in fp32, as two separately rounded operations.  The
// inner-product pass forms y on the fly and the update pass stores it: both go through this one helper, with contraction into an fma switched off,
// so the products are taken against exactly the stored bits on every path (16-byte and scalar) and for every grad_scale.
__device__ __forceinline__ void scaled_grad_and_y(float gs, float g, float gk, float& gn, float& y) {
#pragma clang fp contract(off)
    gn = gs * g;
    y = gn - gk;
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o >= 1; o >>= 1) { const double t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}

__global__ __launch_bounds__(256) void init_kernel(char* state, InitArgs a) {
    Header* h = reinterpret_cast<Header*>(state);       // (the buffer was zeroed in front of this launch)
    const int tid = threadIdx.x;
    if (tid < MAX_SUMS) h->coeff[tid] = tid < a.n_sums ? (double)a.coeff[tid] : 0.0;
    if (tid == 0) {
        h->P = a.P; h->m = a.m; h->n_sums = a.n_sums; h->maxiter = a.maxiter; h->maxfun = a.maxfun; h->maxls = a.maxls;
        h->grad_scale = a.grad_scale; h->ftol = a.ftol; h->gtol = a.gtol;
        long long g = (a.P + 1023) / 1024;
        g = g < 1 ? 1 : (g > GRID ? GRID : g);
        h->gactive = (int)g;
        h->chunk = (int)((((a.P + g - 1) / g) + 3) & ~3LL);
        h->gamma = 1.0;
    }
}

// ---- pass 1: every inner product of the update ---------------------------------------------------------------------------------------------
// Block b owns the elements [b * chunk, (b + 1) * chunk); its four waves share the work units (one history row each, then the scalars);
// a lane accumulates in fp64 over its elements, the wave adds its 64 lanes in a fixed butterfly, lane 0 writes the block's partial.
template <int W>
__device__ __forceinline__ void row_sweep(const float* row, const float* grad, const float* gk, long len, int lane, float gs, double& a0, double& a1) {
    for (long i = (long)lane * W; i + W <= len; i += 64 * W) {
        float r[W], g[W], k[W];
        ld<W>(row + i, r); ld<W>(grad + i, g); ld<W>(gk + i, k);
        for (int e = 0; e < W; ++e) {
            float gn, y;
            scaled_grad_and_y(gs, g[e], k[e], gn, y);
            a0 += (double)r[e] * (double)gn;
            a1 += (double)r[e] * (double)y;
        }
    }
}

template <int W>
__device__ __forceinline__ void scal_sweep(const float* xn, const float* grad, const float* xk, const float* gk, const float* d, long len, int lane, float gs,
                                           double* acc) {
    for (long i = (long)lane * W; i + W <= len; i += 64 * W) {
        float x[W], g[W], xo[W], go[W], dd[W];
        ld<W>(xn + i, x); ld<W>(grad + i, g); ld<W>(xk + i, xo); ld<W>(gk + i, go); ld<W>(d + i, dd);
        for (int e = 0; e < W; ++e) {
            float gn, y;
            scaled_grad_and_y(gs, g[e], go[e], gn, y);
            const float s = x[e] - xo[e];
            acc[Q_SY] += (double)s * (double)y;
            acc[Q_YY] += (double)y * (double)y;
            acc[Q_SG] += (double)s * (double)gn;
            acc[Q_YG] += (double)y * (double)gn;
            acc[Q_GG] += (double)gn * (double)gn;
            acc[Q_GD] += (double)gn * (double)dd[e];
            const double ag = __builtin_fabs((double)gn);
            if (__builtin_isfinite(gn)) acc[Q_GMAX] = ag > acc[Q_GMAX] ? ag : acc[Q_GMAX];
            else acc[Q_BAD] += 1.0;
        }
    }
}

__global__ __launch_bounds__(256) void dots_kernel(char* state, const float* xnew, const float* grad, int vec) {
    const Header* h = reinterpret_cast<const Header*>(state);
    if (h->rec.status != ST_RUNNING) return;
    const int b = blockIdx.x;
    if (b >= h->gactive) return;
    const long long P = h->P;
    const Layout L = make_layout(P, h->m);
    const long lo = (long)b * h->chunk;
    long len = (long)(P - lo < h->chunk ? P - lo : h->chunk);
    if (len < 0) len = 0;
    const long len4 = vec ? (len & ~3L) : 0;             // 16-byte part, then the scalar tail
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = h->rec.pairs;
    const float gs = h->grad_scale;
    double* part = reinterpret_cast<double*>(state + L.part) + (size_t)b * QMAX;
    const float* xk = reinterpret_cast<const float*>(state + L.x) + lo;
    const float* gk = reinterpret_cast<const float*>(state + L.g) + lo;
    const float* d = reinterpret_cast<const float*>(state + L.d) + lo;
    const float* S = reinterpret_cast<const float*>(state + L.S) + lo;
    const float* Y = reinterpret_cast<const float*>(state + L.Y) + lo;
    for (int u = wave; u <= 2 * n; u += 4) {
        if (u < 2 * n) {
            const int j = u >> 1, isy = u & 1;
            const float* row = (isy ? Y : S) + (size_t)j * L.stride;
            double a0 = 0.0, a1 = 0.0;
            row_sweep<4>(row, grad + lo, gk, len4, lane, gs, a0, a1);
            row_sweep<1>(row + len4, grad + lo + len4, gk + len4, len - len4, lane, gs, a0, a1);
            a0 = wave_sum(a0);
            a1 = wave_sum(a1);
            if (lane == 0) { part[4 * j + 2 * isy] = a0; part[4 * j + 2 * isy + 1] = a1; }
        } else {
            double acc[NSCAL];
            for (int k = 0; k < NSCAL; ++k) acc[k] = 0.0;
            scal_sweep<4>(xnew + lo, grad + lo, xk, gk, d, len4, lane, gs, acc);
            scal_sweep<1>(xnew + lo + len4, grad + lo + len4, xk + len4, gk + len4, d + len4, len - len4, lane, gs, acc);
            for (int k = 0; k < NSCAL; ++k) {
                const double r = k == Q_GMAX ? wave_max(acc[k]) : wave_sum(acc[k]);
                if (lane == 0) part[4 * MAX_M + k] = r;
            }
        }
    }
}

// ---- pass 2: one workgroup -------------------------------------------------------------------------------------------------------------------
// More-Thuente's safeguarded step (MINPACK-2 dcstep).  `ynan`: the far end of the bracket is a point whose loss or gradient was not finite --
// it bounds the interval but carries no values to interpolate with.
__device__ inline void dcstep(double& stx, double& fx, double& dx, double& sty, double& fy, double& dy, double& stp, double fp, double dp, int& brackt,
                              int& ynan, double stpmin, double stpmax) {
    const double sgnd = dp * (dx / __builtin_fabs(dx));
    double stpf, stpc, stpq, theta, s, gamma, p, q, r;
    auto max3 = [](double a, double b, double c) { a = __builtin_fabs(a); b = __builtin_fabs(b); c = __builtin_fabs(c); return a > b ? (a > c ? a : c) : (b > c ? b : c); };
    if (fp > fx) {
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
        s = max3(theta, dx, dp);
        gamma = s * __builtin_sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s));
        if (stp < stx) gamma = -gamma;
        p = (gamma - dx) + theta; q = ((gamma - dx) + gamma) + dp; r = p / q;
        stpc = stx + r * (stp - stx);
        stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx);
        stpf = __builtin_fabs(stpc - stx) < __builtin_fabs(stpq - stx) ? stpc : stpc + (stpq - stpc) / 2.0;
        brackt = 1;
    } else if (sgnd < 0.0) {
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
        s = max3(theta, dx, dp);
        gamma = s * __builtin_sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s));
        if (stp > stx) gamma = -gamma;
        p = (gamma - dp) + theta; q = ((gamma - dp) + gamma) + dx; r = p / q;
        stpc = stp + r * (stx - stp);
        stpq = stp + (dp / (dp - dx)) * (stx - stp);
        stpf = __builtin_fabs(stpc - stp) > __builtin_fabs(stpq - stp) ? stpc : stpq;
        brackt = 1;
    } else if (__builtin_fabs(dp) < __builtin_fabs(dx)) {
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
        s = max3(theta, dx, dp);
        double t = (theta / s) * (theta / s) - (dx / s) * (dp / s);
        gamma = s * __builtin_sqrt(t > 0.0 ? t : 0.0);
        if (stp > stx) gamma = -gamma;
        p = (gamma - dp) + theta; q = (gamma + (dx - dp)) + gamma; r = p / q;
        if (r < 0.0 && gamma != 0.0) stpc = stp + r * (stx - stp);
        else stpc = stp > stx ? stpmax : stpmin;
        stpq = stp + (dp / (dp - dx)) * (stx - stp);
        if (brackt) {
            stpf = __builtin_fabs(stpc - stp) < __builtin_fabs(stpq - stp) ? stpc : stpq;
            const double lim = stp + 0.66 * (sty - stp);
            if (stp > stx) stpf = lim < stpf ? lim : stpf;
            else stpf = lim > stpf ? lim : stpf;
        } else {
            stpf = __builtin_fabs(stpc - stp) > __builtin_fabs(stpq - stp) ? stpc : stpq;
            stpf = stpmax < stpf ? stpmax : stpf;
            stpf = stpmin > stpf ? stpmin : stpf;
        }
    } else {
        if (brackt && ynan) {
            stpf = stp + 0.5 * (sty - stp);
        } else if (brackt) {
            theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp;
            s = max3(theta, dy, dp);
            gamma = s * __builtin_sqrt((theta / s) * (theta / s) - (dy / s) * (dp / s));
            if (stp > sty) gamma = -gamma;
            p = (gamma - dp) + theta; q = ((gamma - dp) + gamma) + dy; r = p / q;
            stpf = stp + r * (sty - stp);
        } else {
            stpf = stp > stx ? stpmax : stpmin;
        }
    }
    if (fp > fx) {
        sty = stp; fy = fp; dy = dp; ynan = 0;
    } else {
        if (sgnd < 0.0) { sty = stx; fy = fx; dy = dx; ynan = 0; }
        stx = stp; fx = fp; dx = dp;
    }
    stp = stpf;
}

constexpr double LS_FTOL = 1e-3, LS_GTOL = 0.9, LS_XTOL = 0.1, LS_STPMAX = 1e10, LS_STPMIN = 0.0;      // scipy's L-BFGS-B (lnsrlb)

__device__ inline void search_start(Header* h, double f, double gd, double stp) {
    h->brackt = 0; h->stage = 1; h->ynan = 0;
    h->finit = f; h->ginit = gd; h->gtest = LS_FTOL * gd;
    h->width = LS_STPMAX - LS_STPMIN; h->width1 = 2.0 * h->width;
    h->stx = 0.0; h->fx = f; h->gx = gd; h->sty = 0.0; h->fy = f; h->gy = gd;
    h->stmin = 0.0; h->stmax = stp + 4.0 * stp;
    h->alpha = stp;
    h->rec.trials = 0;
}

// One dcsrch iteration on the trial (stp, f, g); bad: loss or gradient not finite.  Returns 1 converged (strong Wolfe), 2 ended with a warning,
// 0 continue with h->alpha as the next trial.
__device__ inline int search_step(Header* h, double f, double g, int bad) {
    double stp = h->alpha;
    if (bad) {
        // "too long": the point bounds the bracket from above and the next trial halves the interval
        h->brackt = 1; h->sty = stp; h->ynan = 1;
        stp = h->stx + 0.5 * (stp - h->stx);
    } else {
        const double ftest = h->finit + stp * h->gtest;
        if (h->stage == 1 && f <= ftest && g >= 0.0) h->stage = 2;
        int warn = 0;
        if (h->brackt && (stp <= h->stmin || stp >= h->stmax)) warn = 1;
        if (h->brackt && h->stmax - h->stmin <= LS_XTOL * h->stmax) warn = 1;
        if (stp == LS_STPMAX && f <= ftest && g <= h->gtest) warn = 1;
        if (stp == LS_STPMIN && (f > ftest || g >= h->gtest)) warn = 1;
        if (f <= ftest && __builtin_fabs(g) <= LS_GTOL * (-h->ginit)) return 1;
        if (warn) return 2;
        if (h->stage == 1 && f <= h->fx && f > ftest) {
            const double gt = h->gtest;
            double fm = f - stp * gt, fxm = h->fx - h->stx * gt, fym = h->fy - h->sty * gt, gm = g - gt, gxm = h->gx - gt, gym = h->gy - gt;
            dcstep(h->stx, fxm, gxm, h->sty, fym, gym, stp, fm, gm, h->brackt, h->ynan, h->stmin, h->stmax);
            h->fx = fxm + h->stx * gt; h->fy = fym + h->sty * gt; h->gx = gxm + gt; h->gy = gym + gt;
        } else {
            dcstep(h->stx, h->fx, h->gx, h->sty, h->fy, h->gy, stp, f, g, h->brackt, h->ynan, h->stmin, h->stmax);
        }
    }
    if (h->brackt) {
        if (__builtin_fabs(h->sty - h->stx) >= 0.66 * h->width1) stp = h->stx + 0.5 * (h->sty - h->stx);
        h->width1 = h->width;
        h->width = __builtin_fabs(h->sty - h->stx);
    }
    if (h->brackt) {
        h->stmin = h->stx < h->sty ? h->stx : h->sty;
        h->stmax = h->stx > h->sty ? h->stx : h->sty;
    } else {
        h->stmin = stp + 1.1 * (stp - h->stx);
        h->stmax = stp + 4.0 * (stp - h->stx);
    }
    stp = stp > LS_STPMIN ? stp : LS_STPMIN;
    stp = stp < LS_STPMAX ? stp : LS_STPMAX;
    if ((h->brackt && (stp <= h->stmin || stp >= h->stmax)) || (h->brackt && h->stmax - h->stmin <= LS_XTOL * h->stmax)) stp = h->stx;
    h->alpha = stp;
    if (bad && !(stp > 0.0)) return 2;
    return 0;
}

__device__ __forceinline__ double first_step(double gg) {
    const double nrm = __builtin_sqrt(gg);
    return nrm > 1.0 ? 1.0 / nrm : 1.0;                  // min(1, 1 / ||g||): lnsrlb's first step
}

// Thread 0's decision for this evaluation.  Returns the action of the update pass; a stop sets rec.status (and *restore when the caller's
// parameters have to go back to x_k).
__device__ inline int decide(Header* h, const double* red, const float* sums, double* ring, int* restore) {
    Record& r = h->rec;
    double f = 0.0;
    for (int j = 0; j < h->n_sums; ++j) f += h->coeff[j] * (double)sums[j];
    ring[r.loss_pos % RING] = f;
    r.loss_pos += 1;
    r.evaluations += 1;
    const int bad = !__builtin_isfinite(f) || red[Q_BAD] != 0.0 || !__builtin_isfinite(red[Q_GG]);
    const int out_of_evals = r.evaluations >= h->maxfun;
    *restore = 0;
    if (h->phase == 0) {
        r.f = f; r.gmax = red[Q_GMAX]; r.step = 0.0;
        h->gg = red[Q_GG];
        if (bad) { r.status = ST_NONFINITE_START; return ACT_NONE; }
        if (r.gmax <= h->gtol) { r.status = ST_GTOL; return ACT_NONE; }
        if (out_of_evals) { r.status = ST_MAXFUN; return ACT_NONE; }
        h->phase = 1;
        search_start(h, f, -red[Q_GG], first_step(red[Q_GG]));
        return ACT_INIT;
    }
    r.trials += 1;
    const double stp = h->alpha, ftest = h->finit + stp * h->gtest;
    if (__builtin_isfinite(f) && bad && f <= ftest) {
        // the loss says the point is acceptable, its gradient overflowed: the caller's range ladder has to act (PINN_ADJOINT_SHIFT)
        r.status = ST_NONFINITE_GRAD; *restore = 1; return ACT_NONE;
    }
    int res = search_step(h, f, red[Q_GD], bad);
    if (res == 2 && !bad && f <= ftest) res = 1;         // ended on a warning at a point with sufficient decrease: take it, as lnsrlb does
    if (res == 1) {
        r.iterations += 1;
        r.step = stp;
        const double fold = r.f;
        r.f = f; r.gmax = red[Q_GMAX];
        h->gg = red[Q_GG];
        const double sy = red[Q_SY], yy = red[Q_YY];
        const int skip = sy <= 2.2e-16 * yy;             // scipy's curvature rule: the pair is not stored
        if (skip) r.skipped += 1;
        const double af = __builtin_fabs(fold), an = __builtin_fabs(f);
        const double den = af > an ? (af > 1.0 ? af : 1.0) : (an > 1.0 ? an : 1.0);
        if (r.gmax <= h->gtol) r.status = ST_GTOL;
        else if ((fold - f) / den <= h->ftol) r.status = ST_FTOL;
        else if (r.iterations >= h->maxiter) r.status = ST_MAXITER;
        else if (out_of_evals) r.status = ST_MAXFUN;
        // a stop: the caller's parameters are the accepted point already; the update pass does not run, so the last step's pair is not stored
        // and the ring's bookkeeping stays what it is (pairs held == rows debug_read returns)
        if (r.status != ST_RUNNING) return ACT_NONE;
        h->slot = -1;
        if (!skip) {
            if (r.pairs < h->m) { h->slot = r.pairs; r.pairs += 1; }
            else { h->slot = h->head; h->head = (h->head + 1) % h->m; }
            h->gamma = sy / yy;
        }
        return ACT_ACCEPT;
    }
    if (res == 2 || r.trials >= h->maxls) {
        // line search failed: once per iterate, drop the history and search along -g_k (lnsrlb's restart); then give up
        if (r.pairs > 0 && !h->restarted && !out_of_evals) {
            h->restarted = 1;
            r.pairs = 0; h->head = 0; h->gamma = 1.0;
            search_start(h, r.f, -h->gg, first_step(h->gg));
            return ACT_RESTART;
        }
        r.status = out_of_evals ? ST_MAXFUN : ST_LINESEARCH;
        *restore = 1;
        return ACT_NONE;
    }
    if (out_of_evals) { r.status = ST_MAXFUN; *restore = 1; return ACT_NONE; }
    return ACT_TRIAL;
}

__global__ __launch_bounds__(256) void solve_kernel(char* state, float* params, const float* sums, int vec) {
    __shared__ double red[QMAX];
    __shared__ double R[MAX_M * MAX_M];
    __shared__ double u[MAX_M], w[MAX_M], rhs[MAX_M];
    __shared__ int s_act[2];
    Header* h = reinterpret_cast<Header*>(state);
    if (h->rec.status != ST_RUNNING) return;             // after a stop nothing is written any more
    const int tid = threadIdx.x;
    const Layout L = make_layout(h->P, h->m);
    const int n_old = h->rec.pairs, ga = h->gactive;
    const double* part = reinterpret_cast<const double*>(state + L.part);
    for (int q = tid; q < QMAX; q += 256) {              // second stage: block partials in block order
        const int held = q < 4 * MAX_M ? (q >> 2) < n_old : 1;
        double v = 0.0;
        if (held) {
            for (int b = 0; b < ga; ++b) {
                const double t = part[(size_t)b * QMAX + q];
                v = q == 4 * MAX_M + Q_GMAX ? (t > v ? t : v) : v + t;
            }
        }
        red[q] = v;
    }
    __syncthreads();
    if (tid == 0) {
        int restore = 0;
        s_act[0] = decide(h, red + 4 * MAX_M, sums, reinterpret_cast<double*>(state + L.ring), &restore);
        s_act[1] = restore;
        h->action = s_act[0];
    }
    __syncthreads();
    const int act = s_act[0];
    if (s_act[1]) {
        // a stop away from an accepted point: the caller's parameters go back to x_k (done here, so that later calls write nothing at all)
        const float* xk = reinterpret_cast<const float*>(state + L.x);
        for (long long i = tid; i < h->P; i += 256) params[i] = xk[i];
        return;
    }
    if (act != ACT_ACCEPT) return;
    (void)vec;
    double* SY = reinterpret_cast<double*>(state + L.sy);
    double* YY = reinterpret_cast<double*>(state + L.yy);
    const int n = h->rec.pairs, slot = h->slot, m = h->m;
    const double* sc = red + 4 * MAX_M;
    // S^T g, Y^T g at the new x_k, and the new pair's column of S^T Y / row and column of Y^T Y (against the stored fp32 pair)
    if (tid < n) {
        const int j = tid;
        if (j == slot) {
            h->p[j] = sc[Q_SG]; h->q[j] = sc[Q_YG];
            SY[j * MAX_M + j] = sc[Q_SY]; YY[j * MAX_M + j] = sc[Q_YY];
        } else {
            h->p[j] = red[4 * j]; h->q[j] = red[4 * j + 2];
            if (slot >= 0) {
                SY[j * MAX_M + slot] = red[4 * j + 1];
                YY[j * MAX_M + slot] = red[4 * j + 3]; YY[slot * MAX_M + j] = red[4 * j + 3];
            }
        }
    }
    if (tid < MAX_M) { h->a[tid] = 0.0; h->b[tid] = 0.0; }
    __syncthreads();
    if (n == 0) {                                        // no pair held (the first ones were skipped): steepest descent
        if (tid == 0) { h->gamma = 1.0; h->restarted = 0; search_start(h, h->rec.f, -h->gg, first_step(h->gg)); }
        return;
    }
    // logical (age) order k = 0 .. n-1, oldest first -> ring slot
    const int start = n == m ? h->head : 0;
    auto phys = [&](int k) { return (start + k) % m; };
    const double gamma = h->gamma;
    for (int e = tid; e < n * n; e += 256) {
        const int k = e / n, l = e % n;
        R[k * MAX_M + l] = l >= k ? SY[phys(k) * MAX_M + phys(l)] : 0.0;
    }
    if (tid < n) rhs[tid] = h->p[phys(tid)];
    __syncthreads();
    for (int k = n - 1; k >= 0; --k) {                   // u = R^-1 p   (R = triu(S^T Y))
        if (tid == 0) u[k] = rhs[k] / R[k * MAX_M + k];
        __syncthreads();
        if (tid < k) rhs[tid] -= R[tid * MAX_M + k] * u[k];
        __syncthreads();
    }
    if (tid < n) {                                       // w = (D + gamma Y^T Y) u - gamma q
        const int k = tid;
        double v = 0.0;
        for (int l = 0; l < n; ++l) v += YY[phys(k) * MAX_M + phys(l)] * u[l];
        w[k] = R[k * MAX_M + k] * u[k] + gamma * v - gamma * h->q[phys(k)];
    }
    __syncthreads();
    if (tid < n) rhs[tid] = w[tid];
    __syncthreads();
    for (int k = 0; k < n; ++k) {                        // a = R^-T w
        if (tid == 0) w[k] = rhs[k] / R[k * MAX_M + k];
        __syncthreads();
        if (tid > k && tid < n) rhs[tid] -= R[k * MAX_M + tid] * w[k];
        __syncthreads();
    }
    if (tid < n) { h->a[phys(tid)] = w[tid]; h->b[phys(tid)] = -u[tid]; }
    __syncthreads();
    if (tid == 0) {
        // g.d of the new direction from the same products: d = -(gamma g + S a + gamma Y b)
        double gd = gamma * h->gg;
        for (int k = 0; k < n; ++k) gd += w[k] * h->p[phys(k)] + gamma * (-u[k]) * h->q[phys(k)];
        gd = -gd;
        h->restarted = 0;
        if (!(gd < 0.0)) {
            // not a descent direction (cannot happen in exact arithmetic): drop the history, steepest descent
            for (int k = 0; k < MAX_M; ++k) { h->a[k] = 0.0; h->b[k] = 0.0; }
            h->rec.pairs = 0; h->head = 0; h->gamma = 1.0; h->slot = -1;
            search_start(h, h->rec.f, -h->gg, first_step(h->gg));
        } else {
            search_start(h, h->rec.f, gd, 1.0);
        }
    }
}

// ---- pass 3: history, iterate, direction, next trial point ---------------------------------------------------------------------------------------
template <int W>
__device__ __forceinline__ void update_elems(char* state, const Header* h, const Layout& L, float* params, const float* grad, long i, int act) {
    float* xk = reinterpret_cast<float*>(state + L.x) + i;
    float* gk = reinterpret_cast<float*>(state + L.g) + i;
    float* dv = reinterpret_cast<float*>(state + L.d) + i;
    float* S = reinterpret_cast<float*>(state + L.S) + i;
    float* Y = reinterpret_cast<float*>(state + L.Y) + i;
    const double alpha = h->alpha;
    float x[W], d[W], out[W];
    if (act == ACT_TRIAL) {
        ld<W>(xk, x); ld<W>(dv, d);
    } else if (act == ACT_RESTART) {
        float g[W];
        ld<W>(xk, x); ld<W>(gk, g);
        for (int e = 0; e < W; ++e) d[e] = -g[e];
        st<W>(dv, d);
    } else {
        float g[W], gn[W], xo[W], go[W], s[W], y[W];
        ld<W>(params + i, x); ld<W>(grad + i, g);
        ld<W>(xk, xo); ld<W>(gk, go);                    // (zeros at ACT_INIT: the state was cleared)
        for (int e = 0; e < W; ++e) {
            scaled_grad_and_y(h->grad_scale, g[e], go[e], gn[e], y[e]);
            s[e] = x[e] - xo[e];                         // the difference of the two points the loss kernels saw
        }
        if (act == ACT_INIT) {
            for (int e = 0; e < W; ++e) d[e] = -gn[e];
        } else {
            const int slot = h->slot, n = h->rec.pairs;
            if (slot >= 0) { st<W>(S + (size_t)slot * L.stride, s); st<W>(Y + (size_t)slot * L.stride, y); }
            const double gamma = h->gamma;
            double acc[W];
            for (int e = 0; e < W; ++e) acc[e] = gamma * (double)gn[e];
            for (int j = 0; j < n; ++j) {
                float sj[W], yj[W];
                if (j == slot) { for (int e = 0; e < W; ++e) { sj[e] = s[e]; yj[e] = y[e]; } }
                else { ld<W>(S + (size_t)j * L.stride, sj); ld<W>(Y + (size_t)j * L.stride, yj); }
                const double aj = h->a[j], bj = gamma * h->b[j];
                for (int e = 0; e < W; ++e) acc[e] += aj * (double)sj[e] + bj * (double)yj[e];
            }
            for (int e = 0; e < W; ++e) d[e] = (float)(-acc[e]);
        }
        st<W>(xk, x); st<W>(gk, gn); st<W>(dv, d);
    }
    for (int e = 0; e < W; ++e) out[e] = (float)((double)x[e] + alpha * (double)d[e]);
    st<W>(params + i, out);
}

__global__ __launch_bounds__(256) void update_kernel(char* state, float* params, const float* grad, int vec) {
    const Header* h = reinterpret_cast<const Header*>(state);
    if (h->rec.status != ST_RUNNING) return;
    const int act = h->action;
    if (act == ACT_NONE) return;
    const long long P = h->P;
    const Layout L = make_layout(P, h->m);
    const long n4 = vec ? (long)(P / 4) : 0;
    const long gt = (long)blockIdx.x * 256 + threadIdx.x, nt = (long)gridDim.x * 256;
    for (long i4 = gt; i4 < n4; i4 += nt) update_elems<4>(state, h, L, params, grad, 4 * i4, act);
    for (long i = 4 * n4 + gt; i < P; i += nt) update_elems<1>(state, h, L, params, grad, i, act);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------
inline int enqueue_init(void* state, const InitArgs& a, size_t total, hipStream_t st) {
    int rc = (int)hipMemsetAsync(state, 0, total, st);
    if (rc) return rc;
    hipLaunchKernelGGL(init_kernel, dim3(1), dim3(256), 0, st, static_cast<char*>(state), a);
    return (int)hipGetLastError();
}

inline int enqueue_advance(void* state, float* params, const float* grad, const float* sums, hipStream_t st) {
    const int vec = ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grad)) & 15) == 0;
    char* s = static_cast<char*>(state);
    hipLaunchKernelGGL(dots_kernel, dim3(GRID), dim3(256), 0, st, s, static_cast<const float*>(params), grad, vec);
    hipLaunchKernelGGL(solve_kernel, dim3(1), dim3(256), 0, st, s, params, sums, vec);
    hipLaunchKernelGGL(update_kernel, dim3(GRID), dim3(256), 0, st, s, params, grad, vec);
    return (int)hipGetLastError();
}

}  // namespace lbfgs
}  // namespace pinn
