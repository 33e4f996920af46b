// The two-scale Lorenz '96 forward map (ces_amd/models.py: lorenz96.solve + statistics, ces/calibrate.py:132-154) over the
// columns of the (p, J) layout: one particle per workgroup of ONE wave.  A particle integrates its own ODE with its own adaptive
// step sequence, so all control flow is wave-uniform and no particle waits for another.  All arithmetic is fp64 whatever the
// engine dtype; the engine dtype governs only how U is read and G written.
//
// Integrator: scipy's RK45 (Dormand-Prince 5(4)) as solve_ivp(method='RK45', max_step=dt, t_eval=t) runs it -- the
// specification is scipy/integrate/_ivp/{rk,common,ivp}.py:
//     select_initial_step (two right-hand sides), then per attempt 6 stages + the FSAL evaluation;
//     error norm = RMS of (K E h) / (atol + rtol max(|y|, |y_new|)), accepted below 1;
//     factor = min(10, 0.9 norm^(-1/5)) (capped at 1 after a rejection) / max(0.2, 0.9 norm^(-1/5));
//     min_step = 10 |nextafter(t) - t|, the step is clipped to T;
//     samples: y + h Q (x, x^2, x^3, x^4), Q = K^T P, at every t_eval in (t_old, t] (the first step takes t_eval = t0 too).
// No trajectory is stored: each sample of the LAST window goes into the five window sums of lorenz96._phi at once, and the
// sample at t[-1] is the carried state.
//
// Placement.  State component i lives in lane i % 64, slot i / 64 (E slots, instantiated for n_state <= 64, 128, 256, 448); y,
// the seven stage vectors and the candidate are registers.  The vector a right-hand side is taken of goes through LDS once
// (cyclic neighbours, the fast-variable sums); the window sums live in LDS behind it, each word owned by one lane.
// The issue's sketch put four independent waves in a workgroup; this is one wave per workgroup (as kernels_darcy.hip):
// the waves would share nothing, a one-wave workgroup's __syncthreads() costs no instruction, and the occupancy limit is the
// register file either way (E = 7: two waves per SIMD).
//
// ONE WAVE PER WORKGROUP is load-bearing (L96_THREADS == 64): LDS accesses of one wave execute in program order, the
// __syncthreads() below only keep the compiler from moving LDS accesses across them.
//
// Every sum has a fixed order (lane-serial, then an xor butterfly whose result is read from lane 0): runs are bit-identical and
// a particle's result does not depend on J, on its column or on its neighbours.  Termination is bounded: status 1 h < min_step
// (scipy's failure), 2 non-finite state or error norm, 3 max_attempts reached; such a particle's outputs are NaN.
#include "cesx_internal.h"
#include "rk45_tables.h"

namespace cesx {

constexpr int L96_THREADS = 64;
static_assert(L96_THREADS == 64, "l96_kernel orders its LDS accesses by the program order of ONE wave");

struct L96Args {
    const void* U; const double* W_in; void* G; double* W_out; int* info; long long J;
    int n_slow, n_fast, n_state, n_obs, stat_mode;
    int par_row[4]; double par_fixed[4];
    double T, max_step, rtol, atol;
    int n_t; const double* t;
    int first_kept;                     // the first sample of the kept window: n_t - window_samples
    int window;
    long long max_attempts;
};

// the same value in every lane: butterfly, then lane 0's (the control flow that follows must be wave-uniform)
__device__ __forceinline__ double l96_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return __shfl(v, 0, 64);
}

struct L96Coef { double F, hc, mcb, c, hcn; };       // F, h c, -c b, c, h c / n_fast

// out = the tendencies of v (_l96_rhs of ces_amd/models.py, its order of operations; no contraction: the host has none)
template <int E>
__device__ __forceinline__ void l96_rhs(double* buf, const double (&v)[E], double (&out)[E], const int (&ks)[E], int lane,
                                        int ns, int nf, int nst, const L96Coef& q) {
#pragma clang fp contract(off)
    __syncthreads();                                  // (one wave: the readers of the previous vector are done)
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane + 64 * e;
        if (i < nst) buf[i] = v[e];
    }
    __syncthreads();
    const int ny = nst - ns;
    const double* Y = buf + ns;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane + 64 * e;
        double r = 0.0;
        if (i < ns) {
            const int km1 = i ? i - 1 : ns - 1, km2 = km1 ? km1 - 1 : ns - 1, kp1 = i + 1 == ns ? 0 : i + 1;
            double s = 0.0;
            for (int l = 0; l < nf; ++l) s += Y[i * nf + l];
            r = (((-buf[km1]) * (buf[km2] - buf[kp1]) - v[e]) + q.F) - q.hc * (s / (double)nf);
        } else if (i < nst) {
            const int j = i - ns;
            const int jp1 = j + 1 == ny ? 0 : j + 1, jp2 = jp1 + 1 == ny ? 0 : jp1 + 1, jm1 = j ? j - 1 : ny - 1;
            r = ((q.mcb * Y[jp1]) * (Y[jp2] - Y[jm1]) - q.c * v[e]) + q.hcn * buf[ks[e]];
        }
        out[e] = r;
    }
}

// sqrt(sum x^2) / sqrt(n) over the whole state (common.py norm); ``ss``: this lane's sum of squares
__device__ __forceinline__ double l96_norm(double ss, double sqrt_n) { return sqrt(l96_wave_sum(ss)) / sqrt_n; }

template <typename T, int E>
__global__ __launch_bounds__(L96_THREADS)
void l96_kernel(const L96Args a) {
    extern __shared__ double l96_smem[];
    const int lane = threadIdx.x;
    const long long j = blockIdx.x;                       // the particle
    const int ns = a.n_slow, nf = a.n_fast, nst = a.n_state;
    double* buf = l96_smem;                               // [n_state] the vector a right-hand side (or a sample's sums) is taken of
    double* st = l96_smem + nst;                          // [5][n_slow] window sums, word (b, k) owned by lane k % 64
    const T* U = (const T*)a.U;
    T* G = (T*)a.G;

    double par[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) par[s] = a.par_row[s] >= 0 ? (double)U[(size_t)a.par_row[s] * a.J + j] : a.par_fixed[s];
    L96Coef q;
    {
        const double h = par[0], c = exp(par[2]), b = par[3];
        q.F = par[1]; q.hc = h * c; q.mcb = (-c) * b; q.c = c; q.hcn = (h * c) / (double)nf;
    }
    int ks[E];
    double y[E], K[7][E], yn[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane + 64 * e;
        ks[e] = i >= ns && i < nst ? (i - ns) / nf : 0;
        y[e] = i < nst ? a.W_in[(size_t)i * a.J + j] : 0.0;
    }
    for (int k = lane; k < 5 * ns; k += L96_THREADS) st[k] = 0.0;

    const double rtol = a.rtol, atol = a.atol, Tend = a.T, sqrt_n = sqrt((double)nst);
    int status = 0, n_acc = 0;
    long long n_att = 0;

    // ---- select_initial_step (common.py:68-134), order = 4 ----
    l96_rhs<E>(buf, y, K[0], ks, lane, ns, nf, nst, q);
    double h_abs;
    {
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const double sc = atol + fabs(y[e]) * rtol, u = y[e] / sc, w = K[0][e] / sc;
            s0 += u * u; s1 += w * w;
        }
        const double d0 = l96_norm(s0, sqrt_n), d1 = l96_norm(s1, sqrt_n);
        double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        h0 = fmin(h0, Tend);
#pragma unroll
        for (int e = 0; e < E; ++e) yn[e] = y[e] + h0 * K[0][e];
        l96_rhs<E>(buf, yn, K[1], ks, lane, ns, nf, nst, q);
        double s2 = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const double sc = atol + fabs(y[e]) * rtol, w = (K[1][e] - K[0][e]) / sc;
            s2 += w * w;
        }
        const double d2 = l96_norm(s2, sqrt_n) / h0;
        const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : pow(0.01 / fmax(d1, d2), 0.2);
        h_abs = fmin(fmin(100.0 * h0, h1), fmin(Tend, a.max_step));
        if (!(h_abs == h_abs) || !(d0 - d0 == 0.0)) status = 2;       // a start state or tendencies that are not finite
    }

    // ---- the steps (rk.py:111-176), the samples of each (ivp.py:706-723) ----
    double t = 0.0;
    int si = 0;                                           // the next sample
    const int n_t = a.n_t;
    while (status == 0 && si < n_t) {
        // (all samples lie in [0, T]: t == T implies si == n_t, so an unfinished particle always has a step to take)
        const double min_step = 10.0 * (__longlong_as_double(__double_as_longlong(t) + 1) - t);
        h_abs = h_abs > a.max_step ? a.max_step : (h_abs < min_step ? min_step : h_abs);
        bool rejected = false;
        double h = 0.0, t_new = t;
        for (;;) {
            if (h_abs < min_step) { status = 1; break; }
            if (n_att >= a.max_attempts) { status = 3; break; }
            h = h_abs;
            t_new = t + h;
            if (t_new - Tend > 0.0) t_new = Tend;
            h = t_new - t;
            h_abs = fabs(h);
            ++n_att;
            // rk_step: K[s] = f(y + h (sum_m A[s][m] K[m])), y_new = y + h (sum_m B[m] K[m]), K[6] = f(y_new)
#pragma unroll
            for (int s = 1; s < 6; ++s) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    double dy = 0.0;
#pragma unroll
                    for (int m = 0; m < s; ++m) dy += RK45_A[s][m] * K[m][e];
                    yn[e] = y[e] + dy * h;
                }
                l96_rhs<E>(buf, yn, K[s], ks, lane, ns, nf, nst, q);
            }
#pragma unroll
            for (int e = 0; e < E; ++e) {
                double dy = 0.0;
#pragma unroll
                for (int m = 0; m < 6; ++m) dy += RK45_B[m] * K[m][e];
                yn[e] = y[e] + h * dy;
            }
            l96_rhs<E>(buf, yn, K[6], ks, lane, ns, nf, nst, q);
            double ss = 0.0, bad = 0.0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                double er = 0.0;
#pragma unroll
                for (int m = 0; m < 7; ++m) er += RK45_E[m] * K[m][e];
                const double w = (er * h) / (atol + fmax(fabs(y[e]), fabs(yn[e])) * rtol);
                ss += w * w;
                bad += yn[e] - yn[e];                     // 0, or NaN for a state that is not finite
            }
            const double err = l96_norm(ss, sqrt_n) + l96_wave_sum(bad);
            if (!(err - err == 0.0)) { status = 2; break; }
            const double fac = 0.9 * pow(err, -0.2);
            if (err < 1.0) {
                double factor = err == 0.0 ? 10.0 : fmin(10.0, fac);
                if (rejected) factor = fmin(1.0, factor);
                h_abs *= factor;
                break;
            }
            h_abs *= fmax(0.2, fac);
            rejected = true;
        }
        if (status) break;
        ++n_acc;
        // the samples in (t, t_new] (and t_eval == 0 in the first step): searchsorted(t_eval, t_new, side='right')
        while (si < n_t) {
            const double te = a.t[si];
            if (!(te <= t_new)) break;
            const double x = (te - t) / h, p1 = x, p2 = p1 * x, p3 = p2 * x, p4 = p3 * x;
            double ys[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                double d = 0.0;
                const double pw[4] = {p1, p2, p3, p4};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    double qc = 0.0;
#pragma unroll
                    for (int m = 0; m < 7; ++m) qc += K[m][e] * RK45_P[m][c];
                    d += qc * pw[c];
                }
                ys[e] = h * d + y[e];
            }
            if (si >= a.first_kept) {
                // the five blocks of lorenz96._phi for this sample: X, X^2, mean_l Y, mean_l Y^2, X mean_l Y
                __syncthreads();
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int i = lane + 64 * e;
                    if (i < nst) buf[i] = ys[e];
                }
                __syncthreads();
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int i = lane + 64 * e;
                    if (i < ns) {
                        double s1 = 0.0, s2 = 0.0;
                        for (int l = 0; l < nf; ++l) { const double v = buf[ns + i * nf + l]; s1 += v; s2 += v * v; }
                        const double X = ys[e], yb = s1 / (double)nf, y2 = s2 / (double)nf;
                        st[i] += X; st[ns + i] += X * X; st[2 * ns + i] += yb; st[3 * ns + i] += y2; st[4 * ns + i] += X * yb;
                    }
                }
            }
            if (si == n_t - 1) {                          // ws[-1]: the carried state (W_out may be W_in: this column was read above)
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int i = lane + 64 * e;
                    if (i < nst) a.W_out[(size_t)i * a.J + j] = ys[e];
                }
            }
            ++si;
        }
        t = t_new;
#pragma unroll
        for (int e = 0; e < E; ++e) { y[e] = yn[e]; K[0][e] = K[6][e]; }
    }

    // ---- the observables ----
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const double win = (double)a.window;
    __syncthreads();
    if (a.stat_mode == 0) {
        for (int k = lane; k < 5 * ns; k += L96_THREADS) G[(size_t)k * a.J + j] = (T)(status ? qnan : st[k] / win);
    } else if (lane < 5) {
        double g;
        if (a.stat_mode == 1) {                           // lorenz96_hom: the mean over the slow index
            double s = 0.0;
            for (int k = 0; k < ns; ++k) s += st[lane * ns + k] / win;
            g = s / (double)ns;
        } else {
            g = st[lane * ns + 7] / win;                  // hom = False: slow index 7
        }
        G[(size_t)lane * a.J + j] = (T)(status ? qnan : g);
    }
    if (status) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = lane + 64 * e;
            if (i < nst) a.W_out[(size_t)i * a.J + j] = qnan;
        }
    }
    if (a.info && lane == 0) {
        a.info[j] = status;
        a.info[a.J + j] = n_acc;
        a.info[2 * a.J + j] = (int)(n_att > 0x7fffffffLL ? 0x7fffffffLL : n_att);
        a.info[3 * a.J + j] = 0;
    }
}

template <typename T>
static void l96_launch_T(const L96Args& a, size_t lds, hipStream_t s) {
    const dim3 grid((unsigned)a.J), block(L96_THREADS);
    if (a.n_state <= 64) hipLaunchKernelGGL((l96_kernel<T, 1>), grid, block, lds, s, a);
    else if (a.n_state <= 128) hipLaunchKernelGGL((l96_kernel<T, 2>), grid, block, lds, s, a);
    else if (a.n_state <= 256) hipLaunchKernelGGL((l96_kernel<T, 4>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((l96_kernel<T, 7>), grid, block, lds, s, a);
}

int launch_l96(Engine& e, const void* U, const double* W_in, void* G, double* W_out, int* info, hipStream_t s) {
    const cesx_l96_desc& d = e.l9.desc;
    L96Args a{};
    a.U = U; a.W_in = W_in; a.G = G; a.W_out = W_out; a.info = info; a.J = e.J;
    a.n_slow = d.n_slow; a.n_fast = d.n_fast; a.n_state = d.n_slow * (d.n_fast + 1); a.n_obs = d.n_obs; a.stat_mode = d.stat_mode;
    for (int k = 0; k < 4; ++k) { a.par_row[k] = d.par_row[k]; a.par_fixed[k] = d.par_fixed[k]; }
    a.T = d.T; a.max_step = d.max_step; a.rtol = d.rtol; a.atol = d.atol;
    a.n_t = d.n_t; a.t = e.l9.t;
    a.first_kept = d.n_t - d.window_samples; a.window = d.window_samples;
    a.max_attempts = d.max_attempts;
    if (e.J >= (1LL << 31)) { e.err = "cesx_lorenz_apply: too many particles for one launch"; return CESX_EUNSUPPORTED; }
    const size_t lds = ((size_t)a.n_state + 5 * (size_t)a.n_slow) * 8;       // <= (448 + 5 * 224) * 8 = 12 544 B
    if (e.cfg.dtype == CESX_F32) l96_launch_T<float>(a, lds, s); else l96_launch_T<double>(a, lds, s);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

}  // namespace cesx
