// The Lorenz '63 forward map (ces_amd/models.py: lorenz63.solve after set_solver + statistics, ces/calibrate.py:132-154) over
// the columns of the (p, J) layout: ONE PARTICLE PER LANE.  Three state components, the seven stage vectors, the candidate and
// the nine window sums of a particle are registers of its lane; the kernel uses no LDS, no shuffle, no ballot and no barrier,
// so a lane's result cannot depend on its neighbours, on its column or on J.  (kernels_l96.hip gives a particle a whole wave:
// there the state is up to 448 components and the control flow wave-uniform; here it is per lane.)
//
// Integrator: scipy's RK45 exactly as kernels_l96.hip:6-12 restates it (select_initial_step, 6 stages + FSAL, the RMS error
// norm over the 3 components, the step factors, min_step, clipping to the end time, the dense-output samples at every t_eval),
// with the tables of rk45_tables.h, over [t0, T] = [t[0], t[-1]] as lorenz63.solve passes them to solve_ivp.  All arithmetic is
// fp64 whatever the engine dtype; the engine dtype governs only how U is read and G written.
// What "exactly" covers: the algorithm and its constants.  The right-hand side and the window sums keep the host's order of
// operations with contraction off; the stage, error and dense-output dot products are summed in index order under the
// compiler's default contraction (FMA), where numpy's dot goes through BLAS, and exp() / pow() are the device library's.
// So the outputs are NOT bit-equal to the host's: they agree within the envelope of tests/l63_cases.py (measured on an fp64
// engine: at most 0.2 of its bound), with the host's accepted and attempted step counts in every particle tested.
//
// Control flow.  Every lane runs its own accept / reject sequence in ONE loop whose trip is one attempted step: the lanes of a
// wave share the expensive part (the six right-hand sides) whatever step of whatever particle each is on, and diverge only
// over the samples a step covers.  A lane that has finished or failed leaves the loop and idles until its wave ends.
// Termination is bounded as for Lorenz '96: status 1 h < min_step (scipy's failure), 2 non-finite state or error norm,
// 3 max_attempts reached; such a particle's outputs are NaN.
//
// No trajectory is stored: each sample of the LAST window goes into nine running sums (x, y, z, x^2, y^2, z^2, xy, xz, yz) in
// sample order, and the sample at t[-1] is the carried state.
#include "cesx_internal.h"
#include "rk45_tables.h"

namespace cesx {

constexpr int L63_THREADS = 64;       // one wave per workgroup: the lanes share nothing, a wave that ends frees its slot at once

struct L63Args {
    const void* U; const double* W_in; void* G; double* W_out; int* info; long long J;
    int par_row[3]; double par_fixed[3]; int par_log[3];
    double t0, T, max_step, rtol, atol;
    int n_t; const double* t;
    int first_kept;                     // the first sample of the kept window: n_t - window_samples
    int window;
    long long max_attempts;
};

// the tendencies of v in the order of operations of lorenz63.model (ces_amd/models.py); no contraction: the host has none
__device__ __forceinline__ void l63_rhs(const double (&v)[3], double (&out)[3], double sigma, double r, double b) {
#pragma clang fp contract(off)
    const double x = v[0], y = v[1], z = v[2];
    out[0] = sigma * (y - x);
    out[1] = (r * x - y) - x * z;
    out[2] = x * y - b * z;
}

// sqrt(sum x^2) / sqrt(3) (common.py norm)
__device__ __forceinline__ double l63_norm(double a, double b, double c) { return sqrt((a * a + b * b) + c * c) / sqrt(3.0); }

// np.nextafter(t, inf)
__device__ __forceinline__ double l63_next_up(double t) {
    if (t == 0.0) return __longlong_as_double(1);
    const long long bits = __double_as_longlong(t);
    return __longlong_as_double(t > 0.0 ? bits + 1 : bits - 1);
}

template <typename T>
__global__ __launch_bounds__(L63_THREADS)
void l63_kernel(const L63Args a) {
    const long long j = (long long)blockIdx.x * L63_THREADS + threadIdx.x;       // the particle
    if (j >= a.J) return;                                 // (no barrier below: a lane may leave)
    const T* U = (const T*)a.U;
    T* G = (T*)a.G;

    double par[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        par[s] = a.par_row[s] >= 0 ? (double)U[(size_t)a.par_row[s] * a.J + j] : a.par_fixed[s];
        if (a.par_log[s]) par[s] = exp(par[s]);           // once per particle (the host takes np.exp of the same number every call)
    }
    const double sigma = par[0], r = par[1], b = par[2];
    double y[3], K[7][3], yn[3], sum[9];
#pragma unroll
    for (int e = 0; e < 3; ++e) y[e] = a.W_in[(size_t)e * a.J + j];
#pragma unroll
    for (int k = 0; k < 9; ++k) sum[k] = 0.0;

    const double rtol = a.rtol, atol = a.atol, Tend = a.T, span = fabs(a.T - a.t0);
    int status = 0, n_acc = 0;
    long long n_att = 0;

    // ---- select_initial_step (common.py:68-134), order = 4 ----
    l63_rhs(y, K[0], sigma, r, b);
    double h_abs;
    {
        double u[3], w[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const double sc = atol + fabs(y[e]) * rtol;
            u[e] = y[e] / sc; w[e] = K[0][e] / sc;
        }
        const double d0 = l63_norm(u[0], u[1], u[2]), d1 = l63_norm(w[0], w[1], w[2]);
        double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        h0 = fmin(h0, span);
#pragma unroll
        for (int e = 0; e < 3; ++e) yn[e] = y[e] + h0 * K[0][e];
        l63_rhs(yn, K[1], sigma, r, b);
#pragma unroll
        for (int e = 0; e < 3; ++e) w[e] = (K[1][e] - K[0][e]) / (atol + fabs(y[e]) * rtol);
        const double d2 = l63_norm(w[0], w[1], w[2]) / h0;
        const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : pow(0.01 / fmax(d1, d2), 0.2);
        h_abs = fmin(fmin(100.0 * h0, h1), fmin(span, a.max_step));
        if (!(h_abs == h_abs) || !(d0 - d0 == 0.0)) status = 2;       // a start state or tendencies that are not finite
    }

    // ---- the steps (rk.py:111-176), the samples of each (ivp.py:706-723); one trip = one attempt ----
    double t = a.t0, min_step = 0.0;
    bool fresh = true, rejected = false;                  // fresh: the next attempt is the first of its step
    int si = 0;                                           // the next sample
    const int n_t = a.n_t;
    while (status == 0 && si < n_t) {
        // (all samples lie in [t0, T]: t == T implies si == n_t, so an unfinished particle always has a step to take)
        if (fresh) {
            min_step = 10.0 * fabs(l63_next_up(t) - t);
            h_abs = h_abs > a.max_step ? a.max_step : (h_abs < min_step ? min_step : h_abs);
            rejected = false;
            fresh = false;
        }
        if (h_abs < min_step) { status = 1; break; }
        if (n_att >= a.max_attempts) { status = 3; break; }
        double t_new = t + h_abs;
        if (t_new - Tend > 0.0) t_new = Tend;
        const double h = t_new - t;
        h_abs = fabs(h);
        ++n_att;
        // rk_step: K[s] = f(y + h (sum_m A[s][m] K[m])), y_new = y + h (sum_m B[m] K[m]), K[6] = f(y_new)
#pragma unroll
        for (int s = 1; s < 6; ++s) {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                double dy = 0.0;
#pragma unroll
                for (int m = 0; m < s; ++m) dy += RK45_A[s][m] * K[m][e];
                yn[e] = y[e] + dy * h;
            }
            l63_rhs(yn, K[s], sigma, r, b);
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            double dy = 0.0;
#pragma unroll
            for (int m = 0; m < 6; ++m) dy += RK45_B[m] * K[m][e];
            yn[e] = y[e] + h * dy;
        }
        l63_rhs(yn, K[6], sigma, r, b);
        double w[3], bad = 0.0;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            double er = 0.0;
#pragma unroll
            for (int m = 0; m < 7; ++m) er += RK45_E[m] * K[m][e];
            w[e] = (er * h) / (atol + fmax(fabs(y[e]), fabs(yn[e])) * rtol);
            bad += yn[e] - yn[e];                         // 0, or NaN for a state that is not finite
        }
        const double err = l63_norm(w[0], w[1], w[2]) + bad;
        if (!(err - err == 0.0)) { status = 2; break; }
        const double fac = 0.9 * pow(err, -0.2);
        if (!(err < 1.0)) {                               // rejected: the same step again, shorter
            h_abs *= fmax(0.2, fac);
            rejected = true;
            continue;
        }
        double factor = err == 0.0 ? 10.0 : fmin(10.0, fac);
        if (rejected) factor = fmin(1.0, factor);
        h_abs *= factor;
        ++n_acc;
        // the samples in (t, t_new] (and t_eval == t0 in the first step): searchsorted(t_eval, t_new, side='right')
        double Q[3][4];                                   // K^T P (rk.py _dense_output_impl), once per step
#pragma unroll
        for (int e = 0; e < 3; ++e)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                double qc = 0.0;
#pragma unroll
                for (int m = 0; m < 7; ++m) qc += K[m][e] * RK45_P[m][c];
                Q[e][c] = qc;
            }
        while (si < n_t) {
            const double te = a.t[si];
            if (!(te <= t_new)) break;
            const double x = (te - t) / h;
            const double pw[4] = {x, x * x, (x * x) * x, ((x * x) * x) * x};
            double ys[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                double d = 0.0;
#pragma unroll
                for (int c = 0; c < 4; ++c) d += Q[e][c] * pw[c];
                ys[e] = h * d + y[e];
            }
            if (si >= a.first_kept) {                     // lorenz63.statistics: the nine features of this sample, in sample order
#pragma clang fp contract(off)
                sum[0] += ys[0]; sum[1] += ys[1]; sum[2] += ys[2];
                sum[3] += ys[0] * ys[0]; sum[4] += ys[1] * ys[1]; sum[5] += ys[2] * ys[2];
                sum[6] += ys[0] * ys[1]; sum[7] += ys[0] * ys[2]; sum[8] += ys[1] * ys[2];
            }
            if (si == n_t - 1) {                          // ws[-1]: the carried state (W_out may be W_in: this column was read above)
#pragma unroll
                for (int e = 0; e < 3; ++e) a.W_out[(size_t)e * a.J + j] = ys[e];
            }
            ++si;
        }
        t = t_new;
#pragma unroll
        for (int e = 0; e < 3; ++e) { y[e] = yn[e]; K[0][e] = K[6][e]; }
        fresh = true;
    }

    // ---- the observables ----
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const double win = (double)a.window;
#pragma unroll
    for (int k = 0; k < 9; ++k) G[(size_t)k * a.J + j] = (T)(status ? qnan : sum[k] / win);
    if (status) {
#pragma unroll
        for (int e = 0; e < 3; ++e) a.W_out[(size_t)e * a.J + j] = qnan;
    }
    if (a.info) {
        a.info[j] = status;
        a.info[a.J + j] = n_acc;
        a.info[2 * a.J + j] = (int)(n_att > 0x7fffffffLL ? 0x7fffffffLL : n_att);
        a.info[3 * a.J + j] = 0;
    }
}

int launch_l63(Engine& e, const void* U, const double* W_in, void* G, double* W_out, int* info, hipStream_t s) {
    const cesx_l63_desc& d = e.l6.desc;
    L63Args a{};
    a.U = U; a.W_in = W_in; a.G = G; a.W_out = W_out; a.info = info; a.J = e.J;
    for (int k = 0; k < 3; ++k) { a.par_row[k] = d.par_row[k]; a.par_fixed[k] = d.par_fixed[k]; a.par_log[k] = d.par_log[k] != 0; }
    a.t0 = d.t0; a.T = d.T; a.max_step = d.max_step; a.rtol = d.rtol; a.atol = d.atol;
    a.n_t = d.n_t; a.t = e.l6.t;
    a.first_kept = d.n_t - d.window_samples; a.window = d.window_samples;
    a.max_attempts = d.max_attempts;
    const long long blocks = (e.J + L63_THREADS - 1) / L63_THREADS;
    if (blocks >= (1LL << 31)) { e.err = "cesx_lorenz_three_apply: too many particles for one launch"; return CESX_EUNSUPPORTED; }
    const dim3 grid((unsigned)blocks), block(L63_THREADS);
    if (e.cfg.dtype == CESX_F32) hipLaunchKernelGGL((l63_kernel<float>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((l63_kernel<double>), grid, block, 0, s, a);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

}  // namespace cesx
