/*
 * cesx.h -- C ABI of the MI355X-native EKS / ALDI ensemble-update engine.
 *
 * This is the drop-in boundary for the hot path of agarbuno/ces: the per-step
 * ensemble update of ces/calibrate.py (sampling.eks_update :418-449,
 * sampling.eks_update_aldi :451-490, sampling.eks_update_aldi_constant
 * :492-529 and sampling.timestep_method :243-267).  The reference is pure
 * Python/numpy and has no FFI of its own; each entry point
 * below cites the reference lines whose arithmetic it replaces.  The Python
 * binding a maintainer would add is ces_amd/engine.py (ctypes); see
 * INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no C++ or torch types; all pointers are raw addresses
 *   - "dev" pointers are device (HBM) addresses, "host" pointers host memory
 *   - ensembles keep the reference layout: row-major (p, J), particle index
 *     fastest (ces/calibrate.py:56, 277); a particle shard is a column range
 *   - every call returns CESX_OK (0) or a CESX_E* status; the text of the
 *     last failure is available from cesx_last_error()
 *   - one handle per device, not thread-safe per handle, no global state
 *   - the caller owns every buffer it passes; U is never written
 *     (ces/calibrate.py:357 keeps U0 alive in the trace list)
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     all work is enqueued asynchronously, only cesx_result() waits
 */
#ifndef CESX_H
#define CESX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CESX_ABI_VERSION 10

/* status codes */
#define CESX_OK            0
#define CESX_EINVAL        1   /* bad argument / unknown rule (ValueError)               */
#define CESX_ENOTPD        2   /* covariance not positive definite (np.linalg.LinAlgError,
                                  ces/calibrate.py:446, :487, :526)                      */
#define CESX_EHIP          3   /* HIP runtime failure                                     */
#define CESX_ESTATE        4   /* call order violated (e.g. no problem set)              */
#define CESX_ERCCL         7   /* RCCL failure (cesx_comm_*, cesx_allreduce_*)            */
#define CESX_ENOCONV       6   /* reserved: rounds 1-4 returned it when the Lanczos iteration of
                                  time_step='spectral' missed its residual criterion; since round 5
                                  lambda_max comes from repeated squaring with a two-sided bound and
                                  cannot fail to converge (what np.linalg.eigvals of :250 raises
                                  in that case stays mapped to np.linalg.LinAlgError)          */
#define CESX_EUNSUPPORTED  5   /* time_step='adaptive': the reference calls the undefined
                                  self.LM_procedure (ces/calibrate.py:255)               */

/* arithmetic type of the O(J) passes (moments, update GEMM).  The small dense
   algebra (covariances, Cholesky, gains, time step) always runs in fp64. */
#define CESX_F32 0
#define CESX_F64 1

/* update rule, kwargs['update'] of sampling.run (ces/calibrate.py:304, :364-369) */
#define CESX_UPDATE_EKS            0
#define CESX_UPDATE_ALDI           1
#define CESX_UPDATE_ALDI_CONSTANT  2

/* kwargs['time_step'] of sampling.timestep_method (ces/calibrate.py:247-260) */
#define CESX_TS_DEFAULT   0   /* None: hk = 1/(||D||_F + 1e-8)              :247-248 */
#define CESX_TS_SPECTRAL  1   /* hk = 1/max Re eig(D)                        :249-251 */
#define CESX_TS_CONSTANT  2   /* hk = delta_t                                :252-253 */
#define CESX_TS_ADAPTIVE  3   /* undefined in the reference -> CESX_EUNSUPPORTED :254 */
#define CESX_TS_MIX       4   /* Frobenius until t >= spinup, then delta_t   :256-260 */

typedef struct cesx_engine* cesx_handle;

/* Static shape of one engine = the state of enka.__init__ (ces/calibrate.py:14-22)
   plus the particle shard this device owns. */
typedef struct cesx_config {
    uint32_t struct_bytes;  /* sizeof(cesx_config), for ABI checking                  */
    int32_t  p;             /* parameter dimension            (self.p)                */
    int32_t  n_obs;         /* data dimension                 (self.n_obs)            */
    int32_t  dtype;         /* CESX_F32 | CESX_F64                                    */
    int32_t  device;        /* HIP device ordinal                                     */
    int64_t  J_local;       /* particles held by this device                          */
    int64_t  J_global;      /* ensemble size over all devices (self.J)                */
    int64_t  j_offset;      /* global index of local particle 0 (keys the noise RNG)  */
    uint64_t seed;          /* Philox key for on-device noise                         */
} cesx_config;

/* Per-step options = the **kwargs of eks_update* (ces/calibrate.py:418, 451, 492)
   plus the two pieces of object state the rules read. */
typedef struct cesx_step_params {
    uint32_t struct_bytes;
    int32_t  update;        /* CESX_UPDATE_*                                          */
    int32_t  time_step;     /* CESX_TS_*                                              */
    int32_t  first_step;    /* len(self.Uall) == 1   (ces/calibrate.py:262, :520)     */
    int32_t  t_len;         /* len(self.metrics['t']) before this step   (:257)       */
    int32_t  reserved;
    double   t_last;        /* self.metrics['t'][-1] before this step (if t_len > 0)  */
    double   delta_t;       /* kwargs['delta_t'], default 1/(T/2)        (:253, :260) */
    double   spinup;        /* kwargs['spinup'],  default 4.0            (:257)       */
    double   switch_mult;   /* kwargs['switch'],  default 1.0            (:517)       */
    uint64_t step_index;    /* noise counter: a fresh value per step                  */
} cesx_step_params;

/* What one step appends to the reference's bookkeeping lists. */
typedef struct cesx_step_result {
    double  hk;              /* step size                                            */
    double  t_new;           /* value appended to metrics['t']          (:262-265)   */
    double  self_bias;       /* metrics['self-bias']                    (:432/:464)  */
    double  self_bias_data;  /* metrics['self-bias-data']               (:434/:466)  */
    double  bias_data;       /* metrics['bias-data']                    (:435/:467)  */
    double  bias;            /* metrics['bias']                         (:433/:465)  */
    double  radspec;         /* value appended to self.radspec (spectral only, :250) */
    /* Sharded ensembles: self_bias_data / bias_data above hold only THIS shard's share
       (its sum divided by J_global; the shares of all devices add up to the metric).
       The two fields below are the complete values of the PREVIOUS step: each shard's
       sums ride at the tail of the next step's all-reduced moment buffer, so no second
       collective is needed.  On one device the values above are already complete. */
    double  lag_bias_data;
    double  lag_self_bias_data;
    int32_t status;          /* CESX_OK, CESX_ENOTPD or CESX_ENOCONV for this step; CESX_EHIP:
                                the side stream's factorisation never signalled (one device:
                                its completion is a polled word, bounded; CESX_POLL_JOIN=0 joins
                                with an event instead)                                */
    int32_t reserved;
} cesx_step_result;

/* ---- lifetime -------------------------------------------------------- */

/* Replaces enka.__init__ (ces/calibrate.py:14-22): allocates all device
   workspace for the given shape.  On failure *out is NULL and
   cesx_last_error(NULL) describes why. */
int  cesx_create(const cesx_config* cfg, cesx_handle* out);
void cesx_destroy(cesx_handle h);
const char* cesx_last_error(cesx_handle h);
int  cesx_abi_version(void);

/* Replaces the externally-set object state self.mu, self.sigma, self.ustar
   (examples/scripts/darcy-flow.py:68-75) and the per-call arguments y_obs,
   Gamma of eks_update* (ces/calibrate.py:418).  All HOST pointers to fp64
   arrays: y (n), Gamma (n x n, SPD), mu (p), Sigma (p x p, SPD), ustar (p).
   Factorises Gamma and Sigma once (the reference re-solves them every step,
   ces/calibrate.py:429, :443, :485).
   A DENSE Gamma = L L^T (the reference's pde examples use a sample covariance) is whitened away: once per step the
   engine forms G~ = L^{-1} G (one triangular n x n x J product on the matrix pipe, into an engine-owned n x J buffer
   allocated here) and works with y~ = L^{-1} y, Gamma~ = I -- D = (1/J) E^T Gamma^{-1} R, the data metrics, the gains
   and K (g - y) are invariant (ces/calibrate.py:429-441, :461-473), and every kernel behind it is the diagonal-Gamma
   one.  G_dev itself is never written.  cesx_debug_dense reports gbar and K in the caller's coordinates.
   There is ONE whitened buffer per handle: with a dense Gamma every cesx_moments* call (it whitens G into that buffer) must be
   stream-ordered behind the previous cesx_apply of the handle (whose update kernel reads it) -- the split API's freedom to run
   step i + 1's moments on another stream beside step i's update holds for a diagonal Gamma only.
   Supported conditioning of a dense Gamma on an fp32 engine: the whitening product runs in the engine dtype, its rounding
   eps32 |L^{-1}| |G| is amplified by cond(L) = sqrt(cond(Gamma)) relative to the whitened signal; tests hold cond(Gamma) <= 1e4 with
   |gbar| / spread <= 1e2 to the fp32 bar (tests/test_gpu_parity.py::test_dense_gamma_conditioning); beyond that use an fp64 engine.
   A call that fails (CESX_ENOTPD, an allocation) leaves the handle WITHOUT a problem: nothing is committed before everything is. */
int cesx_set_problem(cesx_handle h, const double* y, const double* Gamma,
                     const double* mu, const double* Sigma, const double* ustar);

/* ---- one step, single device ----------------------------------------- */

/* Replaces one call of sampling.eks_update / eks_update_aldi /
   eks_update_aldi_constant (ces/calibrate.py:418-529) on device-resident
   arrays: U_dev (p x J_local), G_dev (n x J_local) inputs; xi_dev
   (p x J_local) the injected N(0,1) block standing in for
   np.random.normal(0,1,[p,J]) (:447, :488, :527), or NULL to draw it on
   device (Philox4x32-10 keyed by seed, step_index, global particle index);
   U_next_dev (p x J_local) output, must not alias U_dev.  `recenter` != 0
   recomputes the centring shift from the data (required on the first call and
   whenever U/G are unrelated to the previous call). */
int cesx_step(cesx_handle h, const cesx_step_params* prm, const void* U_dev, const void* G_dev,
              const void* xi_dev, void* U_next_dev, int recenter, void* stream);

/* Waits for the last step on this handle and returns what the reference would
   have appended to self.metrics / self.radspec.  Returns CESX_ENOTPD when the
   ensemble covariance was not positive definite (U_next is then undefined).
   (On one device the last small kernel of a step -- fixed-order sum of the data-metric
   partials, copy of the scalars to the host -- is held back so that it can ride on the next
   step's cesx_moments_uu_chol launch; cesx_result, like every entry point that touches the
   engine's state, enqueues it at once if it is still pending.  A driver may therefore enqueue
   the first half of step i+1 before it reads the result of step i, or not: same numbers.
   Lifetime rule that follows: the held-back kernel is enqueued on the `stream` that was passed to
   cesx_apply / cesx_step, so that stream must stay valid until cesx_result (or any other entry
   point of this handle) has been called; what the held-back kernel needs of the moment buffer is
   copied into engine-owned memory by cesx_apply's own kernels.
   Buffers of a step: U_dev, G_dev, xi_dev and U_next_dev must stay valid (and U, G, xi unchanged)
   until cesx_result has returned for that step -- the step is not complete before, and the one
   recovery path below launches its kernels again.  The moment buffer is read by cesx_apply's own
   kernels and, in that recovery alone, once more by cesx_result; a caller may hand it to the next
   step's cesx_moments* before it has read the result (one buffer, pipelined) -- the engine notices,
   and a step whose recovery would need the overwritten buffer reports CESX_EHIP instead of being
   re-run.  ces_amd/dist.py alternates two buffers.) */
int cesx_result(cesx_handle h, cesx_step_result* out);

/* How the caller's stream joins the engine's side stream (centring + chol(C)), and what happens when that goes wrong.
   One device, ALDI, default time step, diagonal Gamma / Sigma: the join is a word the factorisation stores last and one
   workgroup of the caller's stream polls -- ONLY when `stream` has a strictly lower priority than the side stream (two
   streams of one priority level can share a hardware queue, and a waiter queued in front of what it waits for never
   ends); any other stream is joined with an event.  The poll is bounded in wall time (2 s; CESX_POLL_TIMEOUT_MS).  A poll
   that runs out marks the step: its assembly and update launches write NOTHING (U_next, the centring shift and the
   scalars stay as they were), cesx_result switches the engine to the event join for the rest of its life and re-runs
   the step once with chol(C) in line on the caller's stream, from the step's own moment buffer and U / G / xi (see the
   lifetime rules at cesx_result; a moment buffer that a later cesx_moments* call was given in the meantime: no re-run,
   CESX_EHIP).  It then returns CESX_OK -- or CESX_ESTATE when cesx_moments* calls were enqueued after the failed step
   (a pipelined driver): the re-run step's result and U_next are valid, those moments -- and whatever the driver derived
   from the unwritten U_next before, its forward map G first of all -- must be redone (ces_amd/dist.py re-evaluates the
   forward map into the caller's G tensor, then the moments).
   cesx_debug_poll_recoveries: how many steps of this handle were re-run that way. */
unsigned long long cesx_debug_poll_recoveries(cesx_handle h);

/* The hk-dependent SPD inverses of a step -- (Sigma + hk C)^{-1} of the EKS rule (ces/calibrate.py:443), (hk C_gg + Gamma)^{-1} of the
   recomputed gain (:440-441, :472-473) -- are started from the previous step's inverse (Newton-Schulz sweeps on the matrix pipe)
   when that start is close (||I - A X_prev||_F < 0.3) and accepted only when the TRUE residual of the result passes
   (||I - A X||_F < 1e-10); otherwise, and always on the first step of a problem, they are factored from scratch (Cholesky,
   triangular inverse, product).  Same inverse to ~1e-10 either way; CESX_NS_WARM=0 pins the factorisation.
   cesx_debug_warm_inverse: 1 when the last such inverse of this handle was taken from the warm start, else 0.  Synchronises.
   Reproducibility contract: the NUMBER of sweeps a warm start runs is sized from ||I - A X_prev||_F of the last step whose
   result the host has read (cesx_result; reset by cesx_set_problem), and warm and cold inverses agree to ~1e-10, not to the
   bit: chains of these rules are bit-reproducible across call flows that read results at the same cadence (every step, as
   ces_amd's drivers and the reference's loop do -- ces/calibrate.py:387 tests t each iteration); the ranks of a sharded run
   must read in lockstep (ShardedSampler does).  CESX_NS_WARM=0 removes the dependence. */
int cesx_debug_warm_inverse(cesx_handle h);

/* Which form of the update GEMM (ces/calibrate.py:443-447, :484-488, :515-527) the last cesx_apply / cesx_step of this handle
   launched:  0  the assembled coefficient matrix W = [(1 + hk a) I - hk C Sigma^{-1} | -hk K | sqrt(2 hk) L] (every rule, dtype, shape);
              1  ALDI, default time step, fp32: the same matrix with hk kept out of it (the factorisation stores L into the image);
              2  as 1 for a diagonal Sigma and 224 < p <= 256, through the Cholesky factor: C Sigma^{-1} (U - mu) =
                 L (L^T Sigma^{-1} U) - C Sigma^{-1} mu with C = L L^T as factored (:476-478) -- two triangular products instead of
                 the dense one, the intermediate kept in MFMA accumulator registers (CESX_CHAIN=0 keeps form 1).
   The form is chosen by the problem (cesx_set_problem) and the shape alone, never by the call flow.  -1: no handle. */
int cesx_debug_update_form(cesx_handle h);

/* ---- split entry points (multi-device, testing) ----------------------- */

/* Length in doubles of the packed moment buffer that is summed across devices:
   [ N, sum(u-s_u) (p), S_aa (p x p) | sum(g-s_g) (n), S_ab (p x n), S_bb (n x n),
     lagged sum q_r^2, lagged sum q_e^2 (data-metric sums of the previous step) ].
   The first cesx_moments_uu_len() doubles depend on U alone. */
size_t cesx_moments_len(cesx_handle h);
size_t cesx_moments_uu_len(cesx_handle h);

/* Row sums of this shard: sums_dev[0] = J_local, then sum_j U (p), sum_j G (n)
   (fp64).  After summing over devices pass the result to cesx_set_shift. */
int cesx_colsum(cesx_handle h, const void* U_dev, const void* G_dev, double* sums_dev, void* stream);
int cesx_set_shift(cesx_handle h, const double* sums_dev, void* stream);

/* First half of a step (ces/calibrate.py:423-429 / :459-461 / :501-503 and the
   metric sums of :432-435): shifted first and second moments of this shard in
   fp64 into mom_dev (cesx_moments_len doubles).  Additive over shards. */
int cesx_moments(cesx_handle h, const void* U_dev, const void* G_dev, double* mom_dev, void* stream);

/* The same in two pieces, so that chol(C) can start before the Gram is complete:
   cesx_moments_uu fills the leading cesx_moments_uu_len() doubles (N, sum(u-s_u), S_aa -- all
   that cov(U) of ces/calibrate.py:424/:476/:512 needs; a few entries of the second section
   are written too when p is not a multiple of the MFMA tile); cesx_chol_async, called on the
   (summed) leading part, forms C and starts L = chol(C) (:446/:487/:526) on the engine's side
   stream; cesx_moments_rest fills the remainder while that runs; cesx_apply joins.
   cesx_moments = cesx_moments_uu + cesx_moments_rest.  `update` is a CESX_UPDATE_* value
   (it selects the covariance divisor J vs. J-1, :424 vs. :476). */
int cesx_moments_uu(cesx_handle h, const void* U_dev, const void* G_dev, double* mom_dev, void* stream);
int cesx_chol_async(cesx_handle h, int update, const double* mom_dev, void* stream);
int cesx_moments_rest(cesx_handle h, const void* U_dev, const void* G_dev, double* mom_dev, void* stream);
/* cesx_moments_uu + cesx_chol_async in one call, for an ensemble on ONE device (no all-reduce between the two):
   the hand-over to the side stream is then the U x U reduce kernel's own completion signal instead of a marker
   packet in front of the second Gram launch (~6 us per step at C2).  Same results as the two calls. */
int cesx_moments_uu_chol(cesx_handle h, int update, const void* U_dev, const void* G_dev, double* mom_dev, void* stream);
/* The sharded form of the same hand-over: cesx_moments_uu on `stream`, after which the engine's SIDE stream waits
   for it (again through the reduce kernel's own completion signal).  The driver then issues the all-reduce of the
   buffer's head and cesx_chol_async on cesx_side_stream(), and goes on with cesx_moments_rest on `stream`: the
   U x U launch has the device to itself, the collective and chol(C) run beside the second launch. */
int cesx_moments_uu_handover(cesx_handle h, const void* U_dev, const void* G_dev, double* mom_dev, void* stream);

/* ---- the exchange step of a SHARDED ensemble, for callers without torch.distributed ----
   Rank r of N holds the particle columns [j_offset, j_offset + J_local) (cesx_config); per step the packed fp64 moment
   buffer is summed over the ranks -- the only data that crosses GPUs -- by RCCL all-reduces over xGMI, issued on the
   stream the caller names:
       cesx_comm_unique_id   rank 0 draws the 128-byte id (ncclGetUniqueId) and ships it to the others by any host channel
       cesx_comm_init        every rank, collectively: ncclCommInitRank on the handle's device
       cesx_allreduce_head   sum of the leading cesx_moments_uu_len() doubles (N, sum(u - s), S_aa: all chol(C) needs) --
                             between cesx_moments_uu_handover and cesx_chol_async, on cesx_side_stream()
       cesx_allreduce_tail   sum of the rest, behind cesx_moments_rest on the caller's stream
       cesx_allreduce_whole  the north star's literal single all-reduce of the whole buffer (cesx_moments, then this, then
                             cesx_apply factors C in line)
       cesx_allreduce_sum / _max   `count` doubles in place: the first step's centring sums (cesx_colsum) and
                             aldi_constant's max|drift| (ces/calibrate.py:519)
   All in place on device memory, asynchronous on `stream`.  CESX_ERCCL on an RCCL error (text in cesx_last_error).
   librccl.so is bound at run time (a process that already holds a copy keeps using it).  ces_amd/dist.py calls these
   when its engine has a communicator; torch.distributed remains the path of the CPU (gloo) tests. */
#define CESX_COMM_ID_BYTES 128
int cesx_comm_unique_id(void* id_out);
int cesx_comm_init(cesx_handle h, int nranks, int rank, const void* unique_id);
int cesx_comm_destroy(cesx_handle h);
int cesx_comm_nranks(cesx_handle h);                                  /* 0: no communicator */
/* Communicators this handle holds: cesx_comm_init makes TWO where the library has ncclCommSplit -- collectives issued on the
   engine's side stream (cesx_side_stream: the head, beside the second Gram launch) go through the second one, so that no
   communicator is ever used from two streams (CESX_COMM_SPLIT=0: one, shared).  0 / 1 / 2. */
int cesx_comm_count(cesx_handle h);
int cesx_comm_stats(cesx_handle h, unsigned long long* calls, unsigned long long* doubles);   /* all-reduces issued so far, their payload */
int cesx_allreduce_head(cesx_handle h, double* mom_dev, void* stream);
int cesx_allreduce_tail(cesx_handle h, double* mom_dev, void* stream);
int cesx_allreduce_whole(cesx_handle h, double* mom_dev, void* stream);
int cesx_allreduce_sum(cesx_handle h, double* buf_dev, size_t count, void* stream);
int cesx_allreduce_max(cesx_handle h, double* buf_dev, size_t count, void* stream);

/* cesx_moments_rest for a LINEAR forward map (utils.lineal, ces/utils.py:25-31) installed with
   cesx_forward_set_lineal, without a pass over G: with g_j = A u_j + b every G-dependent moment of
   ces/calibrate.py:459-461 / :472 follows from the U-only head of the buffer (N, sum(u-s_u), S_aa) --
   S_ab = S_aa A^T + sa c^T, S_bb = A S_aa A^T + (A sa) c^T + c (A sa)^T + N c c^T, sum(g-s_g) = A sa + N c with
   c = A s_u + b - s_g -- two n x p x p fp64 products instead of the second Gram launch.  mom_dev must hold the
   complete (summed over devices) head; the rest is written, the lagged data-metric sums included.  Valid when
   the G_dev later passed to cesx_apply is what cesx_forward_apply produced from the same U_dev (K3 and the
   per-particle data metrics still read that G).  Not with a dense Gamma (CESX_EUNSUPPORTED: the engine's moments are
   those of the whitened data; take cesx_moments_rest).  The chained device-resident loops of ces_amd use it
   (e2e only; the benchmark's timed step always runs the full Gram). */
int cesx_moments_rest_lineal(cesx_handle h, double* mom_dev, void* stream);

/* The engine's side stream (a hipStream_t).  A sharded driver issues the all-reduce of the
   leading part of the moment buffer on it (and then calls cesx_chol_async with it as
   `stream`), so that collective and chol(C) both run beside cesx_moments_rest without a third
   stream: HIP multiplexes streams onto a few hardware queues, and two streams that share
   one serialise. */
void* cesx_side_stream(cesx_handle h);

/* Second half: small dense algebra on the (summed) moments -- covariance,
   Cholesky, gain, time step (ces/calibrate.py:243-267, :437-446, :469-487) --
   and the fused drift + diffusion update of the shard (:443-447, :484-488). */
int cesx_apply(cesx_handle h, const cesx_step_params* prm, const double* mom_dev,
               const void* U_dev, const void* G_dev, const void* xi_dev,
               void* U_next_dev, void* stream);

/* eks_update_aldi_constant needs max|drift| over the WHOLE ensemble
   (ces/calibrate.py:519).  cesx_apply_drift writes the drift into U_next_dev
   and this shard's max|drift| into absmax_dev[0]; after a max-reduction over
   devices cesx_apply_finish completes U_next = U + hk*drift + sqrt(2hk) L xi. */
int cesx_apply_drift(cesx_handle h, const cesx_step_params* prm, const double* mom_dev,
                     const void* U_dev, const void* G_dev, void* U_next_dev,
                     double* absmax_dev, void* stream);
int cesx_apply_finish(cesx_handle h, const cesx_step_params* prm, const double* absmax_dev,
                      const void* U_dev, const void* xi_dev, void* U_next_dev, void* stream);

/* Noise block the engine would draw for (step_index, shard): fills xi_dev
   (p x J_local).  For tests of the generator. */
int cesx_draw_noise(cesx_handle h, uint64_t step_index, void* xi_dev, void* stream);

/* Optional: draw the noise block of step `step_index` AHEAD of the update, into an engine-owned
   buffer, on the engine's side stream behind the next chol(C) (the f32-input MFMA shares the
   SIMD's vector lanes, so Philox + Box-Muller inside the update kernel cost it matrix-pipe
   cycles).  The engine keeps two such buffers and draws the block of step_index + 1 as well,
   so that a run with consecutive step indices finds every block complete one step ahead
   (CESX_NOISE_LOOKAHEAD=0: one buffer, the step's own block only).  A later cesx_apply /
   cesx_apply_finish / cesx_step with xi_dev == NULL and a matching prm->step_index reads the
   block (same numbers as the in-kernel generator, np.random.normal's role at
   ces/calibrate.py:447/:488/:527); any other step index falls back to drawing inside the
   update kernel.  cesx_step calls it itself. */
int cesx_prefetch_noise(cesx_handle h, uint64_t step_index, void* stream);

/* ---- forward-map hook --------------------------- */

/* G = A U + b for the linear map utils.lineal (ces/utils.py:25-31) evaluated on
   the whole shard at once instead of enka.G_ens' per-particle loop
   (ces/calibrate.py:123-130).  A_dev (n x p, row-major, engine dtype), b_dev
   (n) or NULL. */
int cesx_forward_lineal(cesx_handle h, const void* A_dev, const void* b_dev,
                        const void* U_dev, void* G_dev, void* stream);

/* The same map in two steps for a driver loop that applies ONE map every iteration
   (sampling.run calls model once per particle per iteration, ces/calibrate.py:351-352):
   cesx_forward_set_lineal copies A (and b) into engine-owned buffers laid out for the LDS-DMA
   update kernels, cesx_forward_apply evaluates G = A U + b with them -- no staging copies per
   iteration, and the GEMM runs in the fast kernel.  The engine keeps its own copy: A_dev / b_dev
   may be freed or changed afterwards (call set again to change the map). */
int cesx_forward_set_lineal(cesx_handle h, const void* A_dev, const void* b_dev, void* stream);
int cesx_forward_apply(cesx_handle h, const void* U_dev, void* G_dev, void* stream);

/* ---- forward-map hook: the Darcy flow map of the reference's example (ces/darcy.py and its MATLAB files) ----
   The map of examples/scripts/darcy-flow.py for every column of U at once instead of one MATLAB call per particle
   (ces/calibrate.py:123-130).  For one particle xi (p values), K = Nmesh, m = K - 2:
       L     = coef o Xi, Xi the K x K (row-major) array with Xi[scatter[q]] = xi[q] and zeros elsewhere, L[0][0] = 0
       theta = D L D^T                 (gaussrnd_coarse.m:6-23: D the orthonormal inverse DCT-II matrix, MATLAB's idct2)
       a     = S exp(theta) S^T        (solve_gwf.m: interp2 'spline' from the cell centres to the K x K nodes)
       A x   = 1                       (5-point operator, arithmetic-mean face coefficients, scaled by (K-1)^2, the m^2 interior
                                        unknowns column by column; half-bandwidth m)
       g_k   = (R' X R'^T)[obs_index[k]],  R' = R[:, 1:-1], X = x as m x m column-major, the K x K centres flattened row-major
   The solve is a banded LU with partial (row) pivoting (LAPACK gbtf2 / gbtrs): the spline of exp(theta) overshoots below zero
   on ordinary inputs and A is then symmetric indefinite.  ALL arithmetic is fp64 whatever the engine dtype, which governs only
   how U_dev is read and G_dev written; every sum runs in a fixed order: two calls are bit-identical.
   These entry points keep state of their own: the linear map of cesx_forward_set_lineal is untouched. */
typedef struct {
    uint32_t struct_bytes;    /* sizeof(cesx_darcy_desc) */
    int32_t K;                /* Nmesh, 4 <= K <= 16 (a not-a-knot spline needs four points; one particle's band must fit in LDS); up to 64 for cesx_darcy_set_streamed */
    int32_t p, n_obs;         /* must equal the handle's p and n_obs; p <= K^2 */
    const double* coef;       /* [K][K] KL coefficients, ALREADY multiplied by K and with entry [0][0] zeroed */
    const int32_t* scatter;   /* [p] the K^2 slot each parameter lands on, distinct (identity: darcy.model; rank[:p]: model_trunc) */
    const double* D;          /* [K][K] row-major */
    const double* S;          /* [K][K] centres -> nodes spline matrix */
    const double* R;          /* [K][K] nodes -> centres spline matrix */
    const int32_t* obs_index; /* [n_obs] picked centres, each in [0, K^2) */
} cesx_darcy_desc;
/* Copies the map (host fp64) into engine-owned memory; replaces an earlier one.  CESX_EINVAL (text in cesx_last_error) for
   K < 4, K > 16, a size mismatch, an index out of range or a repeated scatter index; the installed map is kept then. */
int cesx_darcy_set(cesx_handle h, const cesx_darcy_desc* desc);
/* The same map for 4 <= K <= CESX_DARCY_STREAM_KMAX, installed for the STREAMED solver (kernels_darcy_stream.hip): the banded LU
   keeps only its live window -- (m + 2) x (2 m + 2) entries, m = K - 2 -- in LDS, writes every finished row of U (2 m + 1
   doubles) to an HBM workspace and reads the rows back for the back substitution.  Same descriptor struct, validated exactly
   as cesx_darcy_set validates it but for the upper limit of K; same arithmetic contract and status words.  One persistent
   workgroup per particle in flight; the workspace holds one slot of m^2 (2 m + 1) doubles per workgroup (3 844 000 B at K = 64,
   439 200 B at K = 32):
       slots = max(1, min(J_local, max_workgroups or the automatic grid, CESX_DARCY_WS_CAP / bytes per slot))
   max_workgroups: 0 (automatic: what the device holds at once at this K's LDS size) or the largest grid an apply may launch;
   negative is CESX_EINVAL.  A particle's result depends neither on the grid nor on the slot it ran in.  The failure rule is
   cesx_darcy_set's; each call replaces the map of the other kind too (one Darcy map per handle). */
#define CESX_DARCY_STREAM_KMAX 64
#define CESX_DARCY_WS_CAP ((size_t)1 << 30)   /* bytes: the automatic grid of 256 workgroups at K = 64 (984 064 000 B) stays below it */
int cesx_darcy_set_streamed(cesx_handle h, const cesx_darcy_desc* desc, int max_workgroups);
/* Bytes of HBM workspace the installed map owns: slots m^2 (2 m + 1) 8 for a streamed map, 0 for a resident one or none. */
size_t cesx_darcy_workspace_bytes(cesx_handle h);
/* Dispatches on the kind of the installed map (resident or streamed).
   G_dev (n_obs x J_local) = the installed map of the columns of U_dev (p x J_local), both in the engine dtype.  status_dev
   (J_local int32 on the device, or NULL): 0; or c > 0 -- the pivot of column c (1-based) of that particle was exactly zero, its
   system is singular --; or -c -- column c held a NaN or an infinity when its pivot was sought (exp(theta) overflowed: nothing
   is singular, the input left fp64's range).  The outputs of such a particle are NaN, the other particles are unaffected. */
int cesx_darcy_apply(cesx_handle h, const void* U_dev, void* G_dev, int32_t* status_dev, void* stream);
/* The same map of a RESIDENT installation (cesx_darcy_set) together with the gradient of the data misfit of the sampler's problem
   (cesx_set_problem: y and Gamma, diagonal or dense), by one adjoint solve per particle (kernels_darcy_grad.hip).  The 5-point
   operator A is symmetric, so the adjoint system is a second right-hand side of the factorisation the forward solve has just
   made: the launch keeps the multipliers and the row swaps and runs one more forward and back substitution.  With r = G - y,
   c = Gamma^{-1} r:
       G_dev    [n_obs][J_local] fp64: cesx_darcy_apply's G bit for bit (before an fp32 engine's rounding on the store)
       phid_dev [J_local] fp64:        phi_d = 1/2 r^T c
       dphi_dev [p][J_local] fp64:     d phi_d / d u, through Z.flat[obs] += c, W = R^T Z R, A lambda = interior(W),
                                       d phi_d / d a[s] = -1/2 (K - 1)^2 sum_faces(s, t) (Lambda_s - Lambda_t) (P_s - P_t) and the
                                       transposes of S, exp and D
   U_dev is read in the engine dtype; everything else is fp64 in a fixed order without atomics: two calls are bit-identical.
   status_dev as cesx_darcy_apply's (or NULL); a particle with a non-zero status has NaN in all three outputs.
   CESX_ESTATE without an installed map or without cesx_set_problem; CESX_EUNSUPPORTED for a map installed with
   cesx_darcy_set_streamed (its multipliers are not kept); CESX_EINVAL for a null pointer.  None of these launches anything. */
int cesx_darcy_grad(cesx_handle h, const void* U_dev, double* G_dev, double* phid_dev, double* dphi_dev, int32_t* status_dev,
                    void* stream);
/* Bytes of LDS one workgroup of cesx_darcy_grad takes at this K (the band, the K x K tile and the pivot bytes): 80 648 at K = 16,
   two workgroups per CU.  0 outside 4 .. 16.  Needs no handle and no device. */
size_t cesx_darcy_grad_lds_bytes(int K);

/* ---- forward-map hook: the two-scale Lorenz '96 models of the reference (ces/utils.py:229-448, type == 'pde') ----
   What G_pde (ces/calibrate.py:132-154) does for one particle, for every column at once: integrate the model from the
   carried state over [0, T] with scipy's RK45 as solve_ivp(method='RK45', max_step=dt, t_eval=t) runs it (rtol, atol,
   select_initial_step, the step controller, min_step and the 4th-order dense output of scipy/integrate/_ivp), form the five
   blocks of window statistics X, X^2, mean_l Y, mean_l Y^2, X mean_l Y over the LAST window of window_samples samples (the
   samples 1 + spinup_samples .. n_t - 1 are cut into such windows), and carry the state at t[n_t - 1] on.  One wave per
   particle, fp64 whatever the engine dtype, no atomics, every sum in a fixed order: two calls are bit-identical and a
   particle's result does not depend on J_local, on its column or on the other particles.
   The model's parameters (h, F, log c, b) are each a row of U or a fixed value, which covers lorenz96, lorenz96Fc, lorenz96Fb,
   lorenz96hFb, lorenz96hcb (stat_mode 0, n_obs = 5 n_slow) and lorenz96_hom (stat_mode 1: the blocks averaged over the slow
   index, 2: taken at slow index 7; n_obs = 5).
   These entry points keep state of their own: the lineal and the Darcy maps are untouched. */
typedef struct {
    uint32_t struct_bytes;       /* sizeof(cesx_l96_desc) */
    int32_t n_slow, n_fast;      /* n_slow >= 4, n_fast >= 1, n_state = n_slow (n_fast + 1) <= 448 */
    int32_t n_obs, p;            /* must equal the handle's */
    int32_t stat_mode;           /* 0 per slow index, 1 hom mean, 2 hom index 7 */
    int32_t par_row[4];          /* h, F, log c, b: the row of U, or -1 and ... */
    double par_fixed[4];         /* ... the fixed value */
    double T, max_step, rtol, atol;
    int32_t n_t;                 /* samples */
    const double* t;             /* [n_t] HOST, non-decreasing, within [0, T]; copied */
    int32_t spinup_samples, window_samples;   /* n_t - 1 - spinup_samples is a positive multiple of window_samples */
    int64_t max_attempts;        /* attempted steps after which a particle ends with status 3 (>= 1) */
} cesx_l96_desc;
/* Copies the descriptor; replaces an earlier one.  CESX_EINVAL (text in cesx_last_error) for a shape outside the limits above,
   p / n_obs differing from the handle's, a par_row out of range or repeated, t decreasing or outside [0, T], a sample count
   that does not fill whole windows, or a non-positive T, max_step, rtol, atol; the installed map is kept then. */
int cesx_lorenz_set(cesx_handle h, const cesx_l96_desc* desc);
/* U_dev (p x J_local, engine dtype), W_in_dev (n_state x J_local fp64: the start states) -> G_dev (n_obs x J_local, engine
   dtype), W_out_dev (n_state x J_local fp64: the states at t[n_t - 1]; may equal W_in_dev).  G_dev must not alias U_dev.
   info_dev ([4][J_local] int32 on the device, or NULL): row 0 the status -- 0; 1 the step fell below min_step (scipy's
   "required step size is less than spacing between numbers"); 2 a state or an error norm was not finite; 3 max_attempts
   steps were attempted --, row 1 the accepted steps, row 2 the attempted steps, row 3 zero.  The outputs of a particle with
   a status other than 0 are NaN, the other particles are unaffected.  Where t[n_t - 1] < T a particle stops once its last
   sample is out. */
int cesx_lorenz_apply(cesx_handle h, const void* U_dev, const double* W_in_dev, void* G_dev, double* W_out_dev,
                   int32_t* info_dev, void* stream);

/* ---- forward-map hook: the Lorenz '63 models of the reference (ces/utils.py:124-227, type == 'pde') ----
   What G_pde (ces/calibrate.py:132-154) does for one particle of lorenz63 / lorenz63_log, for every column at once, with the
   integrator ces_amd.models.lorenz63.set_solver selects: scipy's RK45 as solve_ivp(fun, [t[0], t[-1]], w0, t_eval=t,
   max_step=, rtol=, atol=) runs it (the restatement of cesx_lorenz_apply, the error norm over 3 components), the nine window
   means x, y, z, x^2, y^2, z^2, xy, xz, yz over the LAST window of window_samples samples (the samples 1 .. n_t - 1 are cut
   into such windows), and the state at t[n_t - 1] carried on.  One particle per LANE, each lane with its own accept / reject
   sequence; fp64 whatever the engine dtype, no LDS, no atomics, no exchange between lanes, every sum in sample order: two
   calls are bit-identical and a particle's result does not depend on J_local, on its column or on the other particles.
   (sigma, r, b) are each a row of U or a fixed value; par_log[k] != 0 takes exp() of parameter k once per particle
   (lorenz63_log: r = exp(U[0]), b = exp(U[1])).
   The entry points are spelled cesx_lorenz_three_* (the three-variable Lorenz system; no digit in an entry point's name).
   They keep state of their own: the lineal, the Darcy and the Lorenz '96 maps are untouched. */
typedef struct {
    uint32_t struct_bytes;       /* sizeof(cesx_l63_desc) */
    int32_t par_row[3];          /* sigma, r, b: the row of U (< the handle's p), or -1 and ... */
    double par_fixed[3];         /* ... the fixed value */
    int32_t par_log[3];          /* != 0: the parameter is exp() of the value read */
    double t0, T;                /* the span of the integration, t0 < T (lorenz63.solve: t[0], t[n_t - 1]) */
    double max_step, rtol, atol; /* max_step may be infinite */
    int32_t n_t;                 /* samples */
    const double* t;             /* [n_t] HOST, non-decreasing, within [t0, T]; copied */
    int32_t window_samples;      /* n_t - 1 is a positive multiple of window_samples */
    int64_t max_attempts;        /* attempted steps after which a particle ends with status 3 (>= 1) */
} cesx_l63_desc;
/* Copies the descriptor; replaces an earlier one.  CESX_EINVAL (text in cesx_last_error) for a handle whose n_obs is not 9,
   a par_row out of range or repeated, a fixed parameter that is not finite, t decreasing or outside [t0, T], a sample count
   that does not fill whole windows, t0 >= T or a non-positive max_step, rtol, atol; the installed map is kept then. */
int cesx_lorenz_three_set(cesx_handle h, const cesx_l63_desc* desc);
/* U_dev (p x J_local, engine dtype), W_in_dev (3 x J_local fp64: the start states) -> G_dev (9 x J_local, engine dtype),
   W_out_dev (3 x J_local fp64: the states at t[n_t - 1]; may equal W_in_dev).  G_dev must not alias U_dev.  info_dev
   ([4][J_local] int32 on the device, or NULL) as cesx_lorenz_apply writes it: row 0 the status (0; 1 the step fell below
   min_step; 2 a state or an error norm was not finite; 3 max_attempts steps were attempted), row 1 the accepted steps, row 2
   the attempted steps, row 3 zero.  The outputs of a particle with a status other than 0 are NaN, the other particles are
   unaffected. */
int cesx_lorenz_three_apply(cesx_handle h, const void* U_dev, const double* W_in_dev, void* G_dev, double* W_out_dev,
                            int32_t* info_dev, void* stream);

/* ---- Sample: Metropolis-Hastings over the columns (ces/sample.py) -------
   MCMC.model_mh (ces/sample.py:121-196) runs ONE host chain; here every column of the handle's (p, J_local) layout is an
   independent chain of it (no communication between chains).  Per step:
       cesx_mh_propose   P = a U + b S xi                       (MCMC.random_walk / MCMC.pCN, :198-202)
       (the caller's forward map G_P = G(P): cesx_forward_apply, or any (n x J_local) device array)
       cesx_mh_accept    phi(P), the test log u < phi(U) - phi(P) (:188) and, for the accepted columns, U := P
   with  RW:  a = 1,              b = 1       (S = delta chol(cov(enka.Ustar)) or delta I, :122-126)
         pCN: a = sqrt(1 - beta^2), b = sqrt(beta)  (S = chol(prior.cov), :127-129; the reference's sqrt(beta), :202)
   phi(u) = 1/2 (g - y)^T Gamma^{-1} (g - y) + 1/2 (u - mu)^T Sigma^{-1} (u - mu)   (:141-152 / :170-180; the prior term for
   RW only -- pCN is prior invariant, :143-145; the log-density's constant cancels in the test).  y, Gamma, mu, Sigma are those
   of cesx_set_problem: a dense Gamma is whitened away as in the ensemble update (G_P whitened into the engine's buffer, y~),
   a dense Sigma is scored through w = L_Sigma^{-1} (u - mu), one more triangular p x p x J product per step.  phi and the
   test run in fp64 in a fixed summation order: runs are bit-reproducible.
   Noise (xi_dev / logu_dev NULL): Philox4x32-10 keyed like cesx_draw_noise, but in a counter domain of its own -- the step
   word of every MH draw is step_index | 2^31 (MH step indices must be < 2^31; the ensemble update's steps stay below 2^31), so
   no MH block repeats a block of the ensemble update.  xi rows use the row-quad words 0 .. ceil(p/4) - 1 as cesx_draw_noise does;
   the uniform of chain j is drawn from row-quad word 0xffffffff, which no xi row uses: u = (53 bits of (x, y) + 1/2) 2^-53.
   Unlike the rest of the ABI, cesx_mh_accept WRITES U (the accepted columns).  A later cesx_set_problem drops the proposal
   (cesx_mh_set_proposal again, then cesx_mh_start). */
#define CESX_MH_RW   0
#define CESX_MH_PCN  1
#define CESX_MH_LANGEVIN 2   /* the preconditioned Langevin proposal of cesx_gp_langevin_* (the emulator) and cesx_mh_langevin_* (a
                                closed-form map with its Jacobian, cesx_map_jac), both below; S as for RW, beta ignored.  With
                                this kind cesx_mh_start / _propose / _accept, cesx_gp_start / _accept, cesx_gp_run and
                                cesx_mh_run_map return CESX_EINVAL and launch nothing: they have no gradient of phi. */
/* The proposal: kind CESX_MH_RW | CESX_MH_PCN | CESX_MH_LANGEVIN, S_host the p x p LOWER-triangular scale matrix (row-major fp64, computed by the
   caller exactly as ces/sample.py:122-129 does; CESX_EINVAL when an entry above the diagonal is nonzero), beta the pCN
   parameter (0 < beta <= 1; ignored for RW).  Needs the problem (cesx_set_problem). */
int cesx_mh_set_proposal(cesx_handle h, int kind, const double* S_host, double beta);
/* phi of the current states U_dev (p x J_local) with their forward map G_dev (n x J_local) into engine-owned fp64 memory, and
   the per-chain accept counters cleared.  (ces/sample.py:131-152; a resume that keeps the reference's phi of the start point
   passes the start states here and the resumed states to the steps.) */
int cesx_mh_start(cesx_handle h, const void* U_dev, const void* G_dev, void* stream);
/* P_dev = a U_dev + b S xi (p x J_local, must not alias U_dev); xi_dev the injected N(0,1) block (p x J_local, standing in for
   np.random.normal(0, 1, p) of :199 / :202), or NULL to draw it on device. */
int cesx_mh_propose(cesx_handle h, uint64_t step_index, const void* U_dev, const void* xi_dev, void* P_dev, void* stream);
/* phi(P) from P_dev and G_P_dev = G(P) (n x J_local), the test against logu_dev (J_local fp64 values of log u, standing in for
   np.log(np.random.uniform()) of :188) or, NULL, the device uniform of step_index; accepted columns: U_dev := P_dev, phi
   := phi(P), counter + 1. */
int cesx_mh_accept(cesx_handle h, uint64_t step_index, void* U_dev, const void* P_dev, const void* G_P_dev,
                   const double* logu_dev, void* stream);
/* cesx_mh_accept calls since cesx_mh_start, the overall accept rate (accepted / (steps J_local)) and, per_chain_host != NULL,
   the J_local counters.  Synchronises. */
int cesx_mh_stats(cesx_handle h, unsigned long long* steps, double* rate, unsigned long long* per_chain_host);
/* The J_local current phi values of the chains (fp64, host), as the last start / accept left them; every MH and GP mode.
   Synchronises.  CESX_ESTATE before a start (cesx_mh_start / cesx_gp_start). */
int cesx_mh_phi(cesx_handle h, double* phi_host);

/* ---- Closed-form forward maps over the columns (ces/utils.py:33-122; kernels_maps.hip) --
   The maps of ces_amd.utils.elliptic, banana and the exp prologue of lineal_log, one column per LANE, evaluated in fp64
   whatever the engine dtype and rounded on the store:
       CESX_MAP_ELLIPTIC (prm: x1, x2)  g_i = u2 x_i + exp(-u1) (-x_i^2 + x_i) / 2,  i = 1, 2      (p = n_obs = 2)
       CESX_MAP_BANANA   (prm: a, b)    g_1 = a u1,  g_2 = u2 / a - b (u1^2 + a^2)                 (p = n_obs = 2)
       CESX_MAP_EXP      (no prm)       G = exp(U), (p x J_local) in the engine dtype: lineal_log's prologue, followed by
                                        cesx_forward_apply with the installed lineal map
   The stage keeps state of its own: the lineal, the Darcy and the Lorenz maps and the problem are untouched. */
#define CESX_MAP_ELLIPTIC 1
#define CESX_MAP_BANANA   2
#define CESX_MAP_EXP      3
typedef struct {
    int struct_bytes;            /* sizeof(cesx_map_desc) */
    int kind;                    /* CESX_MAP_* */
    double prm[8];               /* the kind's parameters (above); the rest is ignored */
} cesx_map_desc;
/* Copies the descriptor; replaces an earlier one.  CESX_EINVAL for an unknown kind, a parameter that is not finite (banana:
   a == 0) or a handle whose shape the kind does not fit (elliptic and banana need p = n_obs = 2); the installed map is kept
   then.  Launches nothing. */
int cesx_map_set(cesx_handle h, const cesx_map_desc* desc);
/* U_dev (p x J_local, engine dtype) -> G_dev (n_obs x J_local; CESX_MAP_EXP: p x J_local), engine dtype.  G_dev may equal
   U_dev only for CESX_MAP_EXP.  CESX_ESTATE without an installed map. */
int cesx_map_apply(cesx_handle h, const void* U_dev, void* G_dev, void* stream);
/* n_steps Metropolis steps of every chain in ONE launch, one chain per lane, for the installed map of a fused kind
   (CESX_MAP_ELLIPTIC, CESX_MAP_BANANA): per step k = 0 .. n_steps - 1 the proposal of cesx_mh_propose, the map, phi and the
   test of cesx_mh_accept, with the noise of step step_index + k -- xi_dev[n_steps][p][J_local] (engine dtype) and
   logu_dev[n_steps][J_local] (fp64), or NULL for the device draws of those steps: the counter words of cesx_mh_propose /
   cesx_mh_accept, the normals as an fp64 engine draws them.  Afterwards U_dev, the chains' phi, the accept counters and the
   step count are as n_steps calls of cesx_mh_propose / cesx_map_apply / cesx_mh_accept would have left them (up to the
   rounding of a different order of the same products): fused launches and single steps may alternate.
   trace_dev (NULL: none) receives the states after the steps with (k + 1) % stride == 0, laid out [kept][p][J_local] in the
   engine dtype, kept = n_steps / stride.
   All arithmetic inside a launch is fp64 for either engine dtype; an fp32 engine rounds where it stores -- trace_dev, and
   U_dev at the end of the launch: its state is rounded at launch boundaries only, not after every step.
   CESX_ESTATE without cesx_set_problem, cesx_mh_set_proposal, cesx_mh_start or an installed map of a fused kind; CESX_EINVAL
   for n_steps < 1, stride < 1 or a step index >= 2^31.  Neither launches anything. */
int cesx_mh_run_map(cesx_handle h, uint64_t step_index, int n_steps, int stride, void* U_dev, void* trace_dev,
                    const void* xi_dev, const double* logu_dev, void* stream);
/* G_dev [n_obs][J_local] = the installed map of the columns of U_dev, as cesx_map_apply forms it before it rounds, and
   DG_dev [n_obs][p][J_local], DG[i][q] = dG_i / du_q -- both fp64 whatever the engine dtype, one column per lane: the layout of
   cesx_gp_predict_grad's mean_dev / dmean_dev.
       CESX_MAP_ELLIPTIC   DG = [[-exp(-u1) (-x1^2 + x1) / 2, x1], [-exp(-u1) (-x2^2 + x2) / 2, x2]]      (ces/utils.py:85-86)
       CESX_MAP_BANANA     DG = [[a, 0], [-2 b u1, 1 / a]]
   CESX_ESTATE without an installed map, CESX_EUNSUPPORTED for CESX_MAP_EXP (lineal_log's gradient is an A^T product, not an
   [n][p][J] Jacobian), CESX_EINVAL for a null pointer.  None of these launches anything. */
int cesx_map_jac(cesx_handle h, const void* U_dev, double* G_dev, double* DG_dev, void* stream);
/* MCMC.model_mh(chains=M, update='langevin'): the preconditioned Metropolis-adjusted Langevin step of cesx_gp_langevin_* (below)
   on the TRUE posterior: no cesx_gp_set and no mode.  phi is cesx_mh_start's with the prior term; with G_dev and DG_dev the
   rows and the Jacobian of cesx_map_jac (or any [n][J] / [n][p][J] fp64 images of a forward map and its Jacobian),
       a = Gamma^{-1} (G - y),   grad phi = DG^T a + Sigma_prior^{-1} (u - mu),   g = S^T grad phi
       cesx_mh_langevin_start     phi(U) and g(U); counters cleared
       cesx_mh_langevin_propose   P = U + S (xi - g(U) / 2); the block (xi_dev, or NULL: the device draw of cesx_mh_propose for
                                  step_index) is kept in engine memory
       cesx_mh_langevin_accept    phi(P), g(P) from G_dev, DG_dev at P, then the test
                                      log u < phi(U) - phi(P) + 1/2 |xi|^2 - 1/2 |xi - (g(U) + g(P)) / 2|^2
                                  with cesx_mh_accept's log u; accepted columns: U := P, phi := phi(P), g := g(P), counter + 1
   These are the lv_* kernels of cesx_gp_langevin_* in mode CESX_GP_GAMMA (kernels_gpgrad.hip): a diagonal or a dense
   (whitened) Gamma, a diagonal or a dense prior, NaN rejects.  The counters, cesx_mh_stats and cesx_mh_phi follow.
   CESX_ESTATE without cesx_set_problem, a proposal of kind CESX_MH_LANGEVIN or (propose, accept) a cesx_mh_langevin_start;
   accept also without a propose since the start or the last accept.  CESX_EINVAL for a null pointer, P_dev aliasing U_dev or
   a step index >= 2^31.  None of these launches anything or touches U_dev or the chains' phi. */
int cesx_mh_langevin_start(cesx_handle h, const void* U_dev, const double* G_dev, const double* DG_dev, void* stream);
int cesx_mh_langevin_propose(cesx_handle h, uint64_t step_index, const void* U_dev, const void* xi_dev, void* P_dev, void* stream);
int cesx_mh_langevin_accept(cesx_handle h, uint64_t step_index, void* U_dev, const void* P_dev, const double* G_dev,
                            const double* DG_dev, const double* logu_dev, void* stream);
/* cesx_mh_run_map under a Langevin proposal, for CESX_MAP_ELLIPTIC and CESX_MAP_BANANA: n_steps Langevin steps of every chain in
   ONE launch, one chain per lane, the map, its Jacobian, phi, g and the test above in the lane's registers.  A lane loads
   its state, phi, counter and g (what cesx_mh_langevin_start / _accept left) and stores them once: afterwards U_dev, the
   chains' phi, g, the counters and the step count are as n_steps calls of cesx_mh_langevin_propose / cesx_map_jac /
   cesx_mh_langevin_accept would have left them, so fused launches and single Langevin steps may alternate.  The kernel
   restates the sums of the step path's kernels in their order (g enters the next proposal: a resume that scores the resumed
   states through cesx_mh_langevin_start continues a fused run exactly on an fp64 engine).  Noise, trace_dev, stride and the
   fp32 engine's rounding on the store are cesx_mh_run_map's.
   CESX_ESTATE without cesx_set_problem, a proposal of kind CESX_MH_LANGEVIN, cesx_mh_langevin_start (or cesx_gp_langevin_start)
   or an installed map of a fused kind; CESX_EINVAL for a null U_dev, n_steps < 1, stride < 1 or a step index >= 2^31.
   Neither launches anything. */
int cesx_mh_langevin_run_map(cesx_handle h, uint64_t step_index, int n_steps, int stride, void* U_dev, void* trace_dev,
                             const void* xi_dev, const double* logu_dev, void* stream);
/* The same Langevin step for the LINEAR maps at any p (ces_amd.utils lineal: G = A X + b; lineal_log: G = A exp(X) + b, exp_params
   1), where an [n][p][J] Jacobian image is out of the question: the step needs only the vector-Jacobian product
       t = A^T Gamma^{-1} (G - y)   (lineal_log: exp(X) (.) that),   grad phi = t + Sigma^{-1} (X - mu),   g = S^T grad phi,
   which is a GEMM on the update kernels (kernels_lvlin.hip holds the rest).  phi, the proposal, the test, log u, the noise
   block and its counter words are cesx_mh_langevin_*'s; no log-Jacobian term is added for exp_params.
       cesx_mh_langevin_lineal_set       forms the coefficient images on the host in fp64 from A_host [n_obs][p] and the engine's Gamma,
                                         y, Sigma, mu (cesx_set_problem) and S (cesx_mh_set_proposal), and uploads them.  b_host
                                         ([n_obs] or NULL) is checked and not stored: it reaches the gradient through G_dev alone.
                                         cesx_set_problem and cesx_mh_set_proposal drop the images.  Synchronises.
       cesx_mh_langevin_lineal_start     phi(U) and g(U) from U_dev and G_dev = the map at U ([n_obs][J_local], engine dtype); counters cleared
       cesx_mh_langevin_lineal_propose   P = U + S (xi - g(U) / 2); the block is kept in engine memory
       cesx_mh_langevin_lineal_accept    phi(P), g(P) from G_dev at P, the test, and on the accepted columns U := P, phi := phi(P),
                                         g := g(P), counter + 1.  NaN anywhere in a chain's sums rejects that chain alone.
       cesx_mh_langevin_lineal_g         the chains' g, fp64 on the host, [p][J_local]; synchronises
   phi equals cesx_mh_start's for the same problem bit for bit; g, g(P) and z = xi - g / 2 are [p][J_local] blocks of the engine
   dtype in engine memory.  The two families share phi, the counters, cesx_mh_stats and cesx_mh_phi, but not g: after a
   cesx_mh_langevin_lineal_start, cesx_mh_langevin_propose / _accept / _run_map return CESX_ESTATE until a start of their own,
   and the other way round.
   CESX_ESTATE: set without cesx_set_problem or a proposal of kind CESX_MH_LANGEVIN; start without a set; propose, accept and g
   unless the LAST start was cesx_mh_langevin_lineal_start; accept also without a propose since the start or the last accept.
   CESX_EINVAL for a null pointer (b_host, xi_dev and logu_dev may be NULL), exp_params other than 0 or 1, a non-finite A or b,
   P_dev aliasing U_dev or a step index >= 2^31.  None of these launches anything or touches U_dev, phi or the counters. */
int cesx_mh_langevin_lineal_set(cesx_handle h, const double* A_host, const double* b_host, int exp_params);
int cesx_mh_langevin_lineal_start(cesx_handle h, const void* U_dev, const void* G_dev, void* stream);
int cesx_mh_langevin_lineal_propose(cesx_handle h, uint64_t step_index, const void* U_dev, const void* xi_dev, void* P_dev, void* stream);
int cesx_mh_langevin_lineal_accept(cesx_handle h, uint64_t step_index, void* U_dev, const void* P_dev, const void* G_dev,
                                   const double* logu_dev, void* stream);
int cesx_mh_langevin_lineal_g(cesx_handle h, double* g_host);
/* MCMC.model_mh / gp_mh(chains=M, update='hmc', leapfrog=L): Hamiltonian Monte Carlo with L leapfrog steps per accept test, on
   the pieces of the Langevin step above -- the proposal kind is CESX_MH_LANGEVIN (no kind of its own), the start is
   cesx_mh_langevin_start (a map) or cesx_gp_langevin_start (the emulator), which leave phi and g = S^T grad phi of the chains,
   and phi, g, the noise block, the counters, cesx_mh_stats and cesx_mh_phi are the Langevin step's.  HMC steps, single Langevin
   steps and fused launches of either may therefore alternate on one handle.  With S the scale (the mass matrix is
   (S S^T)^{-1} and the leapfrog step 1: delta is the leapfrog step as it is the Langevin step) one step of a chain at U is
       xi ~ N(0, I_p);   r = xi - g(U) / 2;   Q = U
       l = 1 .. L:   Q = Q + S r;   phi(Q), g(Q);   r = r - g(Q)  (l < L)   or   r = r - g(Q) / 2  (l = L)
       log u < phi(U) - phi(Q) + (|xi|^2 / 2 - |r|^2 / 2);   accepted columns: U := Q, phi := phi(Q), g := g(Q), counter + 1
   At L = 1 this is the Langevin step term for term (r = xi - (g(U) + g(Q)) / 2), and the first position is
   cesx_mh_langevin_propose's P bit for bit.  A step consumes ONE step index whatever L is: the block and log u are the counter
   words of cesx_mh_langevin_propose / _accept for that index, so a run sees the noise of a Langevin run with the same seed.
       cesx_mh_hmc_begin    r (an engine-owned [p][J_local] fp64 block) and the first position Q_dev = U + S r.  The block
                            (xi_dev, engine dtype, or NULL: the device draw for step_index) is kept in engine memory.  Shared
                            by the map and the emulator.  It ends a pending cesx_*_langevin_propose, as such a propose ends a
                            trajectory in flight: both keep their block in the same memory.
       cesx_mh_hmc_leap     phi(Q), g(Q) from G_dev, DG_dev = cesx_map_jac at Q_dev (or any [n][J] / [n][p][J] fp64 images), the
                            full kick, and the next position written over Q_dev.  Called L - 1 times.
       cesx_mh_hmc_accept   phi(Q), g(Q) at the last position, the half kick, the two norms, the test with cesx_mh_accept's log u
       cesx_gp_hmc_leap / cesx_gp_hmc_accept   the same on the rows and gradients of cesx_gp_predict_grad at Q_dev in likelihood
                            mode `mode` (cesx_gp_langevin_*'s modes and their NULL rules)
   r, g, phi and every sum are fp64 in a fixed order (rows ascending): runs are bit-identical.  An fp32 engine stores Q_dev
   rounded after every leapfrog -- the forward map reads that array.  A NaN or an infinity anywhere in a trajectory (phi, g,
   r, Q) makes the comparison false: the chain stays and its phi and g are untouched.
   cesx_mh_hmc_run_map: n_steps such steps of every chain in ONE launch for CESX_MAP_ELLIPTIC and CESX_MAP_BANANA, one chain per
   lane with the trajectory in its registers -- cesx_mh_langevin_run_map with the leapfrog loop inside.  It restates the step
   path's sums in their order: on an fp64 engine it leaves U_dev, phi and g as n_steps times begin / (cesx_map_jac, leap)
   x (L - 1) / cesx_map_jac / accept leave them, bit for bit (a resume that scores the resumed states through
   cesx_mh_langevin_start continues a fused run exactly).  The trajectory is fp64 whatever the engine dtype; an fp32 engine
   rounds on the trace store and at the end of the launch.  Noise, trace_dev and stride are cesx_mh_run_map's.  A launch is
   bounded: n_steps * leapfrog <= CESX_HMC_LAUNCH_GRADS_MAX gradient evaluations.  cesx_mh_stats counts one step per accept
   and n_steps per fused launch.
   CESX_ESTATE without cesx_set_problem, a proposal of kind CESX_MH_LANGEVIN or a cesx_mh_langevin_start /
   cesx_gp_langevin_start as the LAST start (not cesx_mh_langevin_lineal_start: the linear maps have cesx_mh_hmc_lineal_* below); leap and
   accept also without a cesx_mh_hmc_begin since the start or the last accept; the cesx_gp_hmc_* calls without cesx_gp_set;
   run_map without an installed map of a fused kind.  CESX_EINVAL for a null pointer (xi_dev, logu_dev and trace_dev may be
   NULL), Q_dev aliasing U_dev, leapfrog outside 1 .. CESX_HMC_LEAPFROG_MAX, n_steps < 1, stride < 1,
   n_steps * leapfrog > CESX_HMC_LAUNCH_GRADS_MAX, a step index >= 2^31, or what cesx_gp_langevin_* refuses of a mode.  None of
   these launches anything or touches U_dev, the chains' phi, g or the counters. */
#define CESX_HMC_LEAPFROG_MAX 64
#define CESX_HMC_LAUNCH_GRADS_MAX 4096
int cesx_mh_hmc_begin(cesx_handle h, uint64_t step_index, const void* U_dev, const void* xi_dev, void* Q_dev, void* stream);
int cesx_mh_hmc_leap(cesx_handle h, void* Q_dev, const double* G_dev, const double* DG_dev, void* stream);
int cesx_mh_hmc_accept(cesx_handle h, uint64_t step_index, void* U_dev, const void* Q_dev, const double* G_dev,
                       const double* DG_dev, const double* logu_dev, void* stream);
int cesx_gp_hmc_leap(cesx_handle h, int mode, void* Q_dev, const double* mean_dev, const double* var_dev, const double* dmean_dev,
                     const double* dvar_dev, void* stream);
int cesx_gp_hmc_accept(cesx_handle h, int mode, uint64_t step_index, void* U_dev, const void* Q_dev, const double* mean_dev,
                       const double* var_dev, const double* dmean_dev, const double* dvar_dev, const double* logu_dev, void* stream);
int cesx_mh_hmc_run_map(cesx_handle h, uint64_t step_index, int n_steps, int leapfrog, int stride, void* U_dev, void* trace_dev,
                        const void* xi_dev, const double* logu_dev, void* stream);
/* The same leapfrog step for the LINEAR maps at any p (cesx_mh_langevin_lineal_*'s models, images and start; kernels_hmclin.hip):
   every position is update launches -- the gradient g = S^T grad phi as cesx_mh_langevin_lineal_accept forms it, the drift
   Q + S z as cesx_mh_langevin_lineal_propose's triangular launch -- with the momentum r a [p][J_local] block of the ENGINE
   dtype between them (no fp64 momentum image: at p = 256 and 65 536 chains that would be 134 MB more).  One step of a chain
   at U, e = 1 unless the handle is armed (cesx_mh_adapt_set after cesx_mh_langevin_lineal_start):
       xi ~ N(0, I_p);   r = xi - (e / 2) g(U);   Q = U
       L times:   Q = Q + e S r;   G(Q) (the caller's forward map), g(Q);   r = r - e g(Q), the last time r - (e / 2) g(Q)
       log u < phi(U) - phi(Q) + (|xi|^2 / 2 - |r|^2 / 2);   accepted columns: U := Q, phi := phi(Q), g := g(Q), counter + 1
   One step index whatever L is; the block and log u are cesx_mh_langevin_lineal_propose / _accept's for that index.
       cesx_mh_hmc_lineal_begin    r and the first position Q_dev = U + e S r; the block (xi_dev or NULL: the device draw) is kept
       cesx_mh_hmc_lineal_leap     from G_dev = the map at Q_dev: g(Q), the full kick, Qnext_dev = Q + e S r.  phi(Q) is NOT
                                   formed (only the last position's is needed).  Qnext_dev must not alias Q_dev: the drift
                                   launch reads Q while it writes Qnext (ping-pong between two buffers).  Called L - 1 times.
       cesx_mh_hmc_lineal_accept   from G_dev at the last Q_dev: phi(Q), g(Q), the half kick inside the second norm, the test,
                                   the masked copies.  phi is cesx_mh_start's bit for bit.  Unarmed and with no leap since the
                                   begin (L = 1) the launch is cesx_mh_langevin_lineal_accept's own, so L = 1 IS the Langevin
                                   step bit for bit and the two families alternate on one handle.
   A NaN or an infinity anywhere in a trajectory (G, g, r, Q) makes the comparison false: that chain alone stays.
   Armed: the three calls launch the ADAPT instantiations (e from device memory; z = e r is a second block, nothing stored is
   rescaled), accept leaves alpha_j and is followed by the recursion; after n_steps accepts they return CESX_ESTATE.
   CESX_ESTATE without a lineal image or unless the LAST start was cesx_mh_langevin_lineal_start; leap and accept also without a
   cesx_mh_hmc_lineal_begin since the start or the last accept (a cesx_mh_langevin_lineal_propose ends a trajectory in flight).
   CESX_EINVAL for a null pointer (xi_dev, logu_dev may be NULL), Q_dev aliasing U_dev, Qnext_dev aliasing Q_dev, a step index
   >= 2^31.  None of these launches anything or touches U_dev, the chains' phi, g or the counters. */
int cesx_mh_hmc_lineal_begin(cesx_handle h, uint64_t step_index, const void* U_dev, const void* xi_dev, void* Q_dev, void* stream);
int cesx_mh_hmc_lineal_leap(cesx_handle h, const void* Q_dev, const void* G_dev, void* Qnext_dev, void* stream);
int cesx_mh_hmc_lineal_accept(cesx_handle h, uint64_t step_index, void* U_dev, const void* Q_dev, const void* G_dev,
                              const double* logu_dev, void* stream);
/* MCMC.model_mh / gp_mh(chains=M, adapt=): pooled step-size adaptation of the leapfrog step above (kernels_adapt.hip and the
   ADAPT instantiations of kernels_hmc.hip).  One scalar multiplier e, shared by all chains, e_1 = 1.  Adaptation step
   t = 1 .. n_steps is the HMC step with e S in place of S, written without rescaling anything stored (g = S^T grad phi as the
   Langevin step keeps it):
       r = xi - (e / 2) g(U);   Q = U + e S r
       L - 1 times:   phi(Q), g(Q);   r = r - e g(Q);   Q = Q + e S r
       last:          phi(Q), g(Q);   r = r - (e / 2) g(Q)
       d = phi(U) - phi(Q) + (|xi|^2 / 2 - |r|^2 / 2);   accepted iff log u < d
       alpha_j = 1 if d >= 0, exp(d) if d < 0, 0 if d is NaN
   (the Langevin step is L = 1).  Behind the accept, in the same call and on the same stream, ad_update_kernel takes
   abar_t = (1 / M) sum_j alpha_j -- fp64, a fixed order, no atomics -- and
       log e_{t+1} = log e_t + (gain / sqrt(t)) (abar_t - target)
       log ebar_t  = t^-kappa log e_{t+1} + (1 - t^-kappa) log ebar_{t-1},      log ebar_0 = 0
   a Robbins-Monro recursion on the mean acceptance probability with a polynomially weighted average of its iterates.  The
   next step's kernels read e_{t+1} from device memory; stream order hands it over and nothing synchronises with the host
   inside the phase.  The result is multiplier = ebar_{n_steps}.  The draws are the sampler's own: one block and one log u per
   step under the step index the caller passes.
       cesx_mh_adapt_set    after cesx_mh_set_proposal with CESX_MH_LANGEVIN: allocates alpha [J], the state and the history,
                            sets t = 0 and e = 1 and ARMS the handle.  While armed, cesx_mh_hmc_begin / _leap / _accept and
                            cesx_gp_hmc_leap / _accept launch the ADAPT kernels, every accept is followed by the recursion, and
                            after n_steps accepts they return CESX_ESTATE (read, then set the proposal).  While armed,
                            cesx_mh_hmc_run_map, every cesx_*_langevin_propose / _accept / _run_map and the
                            cesx_mh_langevin_lineal_* family return CESX_ESTATE and launch nothing (cesx_mh_hmc_lineal_* is their armed form).  The starts
                            (cesx_mh_langevin_start, cesx_gp_langevin_start) stay available.  cesx_mh_set_proposal and
                            cesx_set_problem disarm the handle and drop the state.
       cesx_mh_adapt_read   synchronises; multiplier = ebar_t of the steps made (1 before the first), steps_done, and into
                            history_host (or NULL) steps_done rows (e_t, abar_t): the multiplier step t ran with and the mean
                            acceptance probability it met.  The handle stays armed.
   CESX_EINVAL: n_steps outside 1 .. CESX_ADAPT_STEPS_MAX, target outside (0, 1), gain <= 0, kappa outside (0.5, 1], a null
   pointer.  CESX_EUNSUPPORTED: a shard (J_local != J_global; pooling across ranks is a reduce this engine does not make).
   CESX_ESTATE: cesx_mh_adapt_set without a proposal of kind CESX_MH_LANGEVIN, cesx_mh_adapt_read on a handle that is not
   armed.  None of these launches anything or touches U_dev, the chains' phi, g or the counters. */
#define CESX_ADAPT_STEPS_MAX 65536
int cesx_mh_adapt_set(cesx_handle h, int n_steps, double target, double gain, double kappa);
int cesx_mh_adapt_read(cesx_handle h, double* multiplier, int* steps_done, double* history_host);
/* Where cesx_mh_langevin_start / _accept and cesx_mh_hmc_leap / _accept take the data term of grad phi from -- an install like
   cesx_mh_adapt_set: no chains, no launch.  For a map whose gradient comes from ONE adjoint solve per state (cesx_darcy_grad) the
   [n][p][J] Jacobian image these calls read is what the adjoint exists to avoid.
       CESX_MH_GRAD_JACOBIAN   (default) DG_dev is the [n_obs][p][J_local] image: everything above, untouched
       CESX_MH_GRAD_READY      DG_dev is a [p][J_local] fp64 block d = d phi_d / du, the data term of grad phi READY-MADE (dphi_dev
                               of cesx_darcy_grad at the same states).  G_dev is still [n_obs][J_local] and phi is still summed
                               from it -- the data sum and the prior of cesx_mh_langevin_start, term for term in their order --,
                                   grad phi = d + Sigma_prior^{-1} (u - mu),   g = S^T grad phi
                               and the kick, the norms, the test, the NaN rule and the masked copies are those of the calls above
                               (the ADAPT forms on an armed handle).  A state whose solve failed has NaN in G_dev and d: rejected
                               like any NaN.  Return codes, the call order, the counters, cesx_mh_stats, cesx_mh_phi and
                               cesx_mh_adapt_* are unchanged; cesx_mh_langevin_propose and cesx_mh_hmc_begin read g alone and are
                               the same launches under either source.  The kernels (kernels_darcy_chain.hip) give a chain one
                               wave, the rows of its triangular products across the lanes, every sum in one fixed order: runs
                               are bit-identical, and leapfrog = 1 is the Langevin step.  p <= 256.
   The source returns to CESX_MH_GRAD_JACOBIAN on every cesx_mh_set_proposal and cesx_set_problem: a sequence that never makes
   this call never sees READY.  The *_run_map, *_lineal_* and cesx_gp_* entry points ignore it.
   CESX_EINVAL: any other source.  CESX_ESTATE: no proposal of kind CESX_MH_LANGEVIN.  CESX_EUNSUPPORTED: READY on an engine
   with p > 256.  It launches nothing and touches neither the chains' phi, g nor the counters. */
#define CESX_MH_GRAD_JACOBIAN 0
#define CESX_MH_GRAD_READY    1
int cesx_mh_grad_source(cesx_handle h, int source);
/* Call order across the families.  The sections above state each family's sequencing against itself; where two of them meet on
   one handle (tests/sampler_reuse_cases.py holds the whole table, state by entry point):
     - One start serves both random-walk families: cesx_mh_accept and cesx_mh_run_map follow a cesx_gp_start, cesx_gp_accept and
       cesx_gp_run a cesx_mh_start.  phi, the counters and the step count are the same memory; the caller answers for scoring
       the proposals with the likelihood the start scored the states with.
     - Under a proposal of kind CESX_MH_LANGEVIN the random-walk calls (cesx_mh_start / _propose / _accept / _run_map, cesx_gp_start /
       _accept / _run) return CESX_EINVAL whether or not a Langevin start has run: the kind is looked at before the start.
     - cesx_mh_langevin_start, cesx_gp_langevin_start and cesx_gp_proj_langevin_start are ONE family: each leaves phi and g in the
       same memory, and cesx_mh_langevin_propose / _accept / _run_map, cesx_gp_langevin_propose / _accept, cesx_gp_proj_langevin_accept
       and the cesx_mh_hmc_* / cesx_gp_hmc_* / cesx_gp_proj_hmc_* calls follow any of the three.  cesx_mh_langevin_lineal_start is the
       other family (g in the engine dtype, in memory of its own): after it only cesx_mh_langevin_lineal_* and cesx_mh_hmc_lineal_*
       step, and after one of the three only the calls above.
     - A start is accepted while a proposal or a trajectory is pending and ends it.
     - cesx_mh_langevin_lineal_set on a handle whose LAST start was cesx_mh_langevin_lineal_start ends that start -- the chains' g
       belonged to the image it replaces --: until the next start every step, cesx_mh_langevin_lineal_g, cesx_mh_phi and
       cesx_mh_stats return CESX_ESTATE.  After one of the other three starts the start stands, and a pending proposal or
       trajectory is ended.
     - cesx_gp_predict and cesx_gp_predict_grad need cesx_gp_set alone, in every state. */

/* ---- Streaming summaries of the chains' draws (MCMC(..., chains=M, summary=True); kernels_chainsum.hip) --
   The sums behind the pooled mean and covariance, the split R-hat and an effective sample size of a run of
   M = J_local chains, taken from the draws while they are in device memory: no draw crosses to the host.  A run
   announces its N draws, adds them in order in any chunking, and reads the sums once.  With n = N / 2 (rounded down),
   a chain's two half-chains are its first n and its last n draws (the middle draw of an odd N belongs to neither):
       per (row, chain, half)   S1 = sum (x - shift), S2 = sum (x - shift)^2, shift = the chain's first draw;
                                m = shift + S1 / n, s^2 = (S2 - S1^2 / n) / (n - 1)
       per row                  W = mean(s^2) and B_m = var(m, ddof = 1) over the 2 M half-chains
       pooled                   c = the row means of the first draw, sum (x - c) and sum (x - c)(x - c)^T over all N M draws
   All sums are fp64 (an fp32 draw converts exactly), run in a fixed order and use no atomics: a run is bit-reproducible,
   and the per-chain sums do not depend on the chunking.
   The stage keeps state of its own, sized by the engine's shape alone, allocated by the first begin and kept until
   cesx_destroy; cesx_set_problem does not touch it.  Its size: the half sums 2 halves x (S1, S2) x p x J_local x 8 bytes
   and the per-chain shift p x J_local x 8 bytes -- 537 MB and 134 MB at p = 256, J_local = 65 536 --, and the pooled
   launch's slab partials, 32 KiB per workgroup of a launch of about 1 024 (34 MB there). */
/* Clears the stage and fixes N = n_draws, and with it the half boundaries.  CESX_EINVAL for n_draws < 4 or a sharded
   handle (J_local != J_global).  Launches nothing. */
int cesx_chain_summary_begin(cesx_handle h, int n_draws, void* stream);
/* Adds `kept` draws laid out [kept][p][J_local] in the engine dtype: a launch's trace_dev (cesx_mh_run_map, cesx_gp_run), or
   U_dev itself with kept = 1.  Reads the draws and writes only the stage's own memory.  CESX_ESTATE without a begin or
   past N draws, CESX_EINVAL for a null pointer or kept < 1; neither launches anything. */
int cesx_chain_summary_add(cesx_handle h, const void* trace_dev, int kept, void* stream);
/* HOST outputs; synchronises `stream`.  c (p), s1 = sum (x - c) (p), cc = sum (x - c)(x - c)^T (p x p row-major, the lower
   triangle; zero above), within = W (p), between = B_m (p); optional (NULL allowed) half_mean and half_var
   ([2 halves][p][J_local] each): m and s^2 of every half-chain.  CESX_ESTATE unless exactly N draws were added (nothing
   is launched then); the stage stays readable until the next begin. */
int cesx_chain_summary_read(cesx_handle h, double* c, double* s1, double* cc, double* within, double* between,
                            double* half_mean, double* half_var, void* stream);

/* ---- Streaming marginals of the chains' draws (MCMC(..., chains=M, summary=True, marginals=...); kernels_chainhist.hip) --
   Histograms of every parameter (row) and of chosen pairs of parameters over all draws of all M = J_local chains, counted
   from the draws while they are in device memory: the input of cesx_chain_summary_add, the other half of its summary.
   The bin rule is fp64 throughout (an fp32 draw converts exactly).  For a row with strictly increasing edges e[0 .. B] a
   draw x lands in bin k where e[k] <= x < e[k + 1], and x == e[B] lands in bin B - 1: what numpy.histogram(x, bins=e)
   counts.  x < e[0] (and -inf) counts as `below`; everything else not inside (x > e[B], +inf, NaN) as `above`; a 2-D draw
   with either coordinate outside goes to the pair's one `outside` counter.  The edges need not be uniform: a guessed bin
   is kept only where the edge array confirms it.
   Counts are integers: a workgroup counts in LDS (32 bits; a launch is cut so that they cannot overflow) and adds what
   it counted to the run's 64-bit totals with integer atomics, so the totals depend neither on the order of the
   workgroups nor on how the run is cut into adds: they are exact, and equal numpy's bit for bit.
   The stage keeps state of its own, sized by p and the caps below alone (not by J_local), allocated by the first begin
   and kept until cesx_destroy; cesx_set_problem does not touch it.  Its size at p = 256 (any J_local, 65 536 included):
   the 1-D totals p x (256 + 2) x 8 bytes = 528 KB and edges p x 257 x 8 bytes = 526 KB, the 2-D totals
   64 pairs x (64 x 64 + 1 outside counter) x 8 bytes = 2.1 MB and edges 64 x 2 x 65 x 8 bytes = 67 KB. */
#define CESX_CHAIN_HIST_BINS_MAX    256
#define CESX_CHAIN_HIST_BINS2D_MAX  64
#define CESX_CHAIN_HIST_PAIRS_MAX   64
typedef struct {
    uint32_t struct_bytes;    /* sizeof(cesx_chain_hist_desc) */
    int32_t bins;             /* B of the 1-D histograms, 2 .. CESX_CHAIN_HIST_BINS_MAX */
    int32_t bins2d;           /* B2 of the 2-D histograms, 2 .. CESX_CHAIN_HIST_BINS2D_MAX */
    int32_t n_pairs;          /* 0 .. CESX_CHAIN_HIST_PAIRS_MAX */
    const double* edges1;     /* HOST [p][bins + 1], every row finite and strictly increasing */
    const double* edges2;     /* HOST [p][bins2d + 1]; only the rows named in `pairs` are read (NULL allowed for n_pairs 0) */
    const int32_t* pairs;     /* HOST [n_pairs][2] rows (i, j), i != j, both in [0, p) (NULL allowed for n_pairs 0) */
} cesx_chain_hist_desc;
/* Starts a run: copies the descriptor and clears the totals (synchronises `stream` first: an earlier run's adds are
   done).  CESX_EINVAL (text in cesx_last_error) for a bad descriptor, a limit above, a pair with i == j or an index outside
   [0, p), edges that are not finite and strictly increasing, or a sharded handle (J_local != J_global); the run in hand,
   if any, goes on unharmed. */
int cesx_chain_hist_begin(cesx_handle h, const cesx_chain_hist_desc* desc, void* stream);
/* Counts `kept` draws laid out [kept][p][J_local] in the engine dtype: the arguments of cesx_chain_summary_add.  Reads
   the draws and writes only the stage's own memory.  CESX_ESTATE without a begin, CESX_EINVAL for a null pointer or
   kept < 1; neither launches anything. */
int cesx_chain_hist_add(cesx_handle h, const void* trace_dev, int kept, void* stream);
/* HOST outputs, all unsigned long long; synchronises `stream`.  hist1 [p][bins]; out1 [p][2] (below, above);
   hist2 [n_pairs][bins2d][bins2d], the row index the bin of the pair's first parameter, the column that of its second;
   out2 [n_pairs] (hist2 and out2 may be NULL for n_pairs 0).  May be called more than once; an add after a read
   continues the run.  CESX_ESTATE without a begin. */
int cesx_chain_hist_read(cesx_handle h, unsigned long long* hist1, unsigned long long* out1, unsigned long long* hist2,
                         unsigned long long* out2, void* stream);

/* ---- Streaming lagged sums of the chains' draws (MCMC(..., chains=M, summary=True, autocorr=...); kernels_chainacf.hip) --
   What an autocorrelation ESS needs of every parameter (row) of the first C = n_chains chains, summed from the draws while
   they are in device memory: the input of cesx_chain_summary_add, a third stage beside it.  All state is fp64 (an fp32 draw
   converts exactly).  For row r, chain j < C and the run's draws x_0 .. x_{N-1}, with the chain's shift c = x_0 and
   a_t = x_t - c, the stage keeps S1 = sum a_t, P_k = sum_{t=0}^{N-1-k} a_t a_{t+k} for k = 0 .. L, and the first and the
   last L of the a_t.  Each P_k is ONE running sum in increasing t (one fma per draw), so the sums do not depend, bit for
   bit, on how the N draws are cut into add calls.  Draws added fewer than 64 at a time wait in the stage's own memory
   (engine dtype) until 64 are there; the sums then move once per block, not once per draw.  read forms, with d = S1 / N,
   Hd_k = S1 - (the last k of a) and Tl_k = S1 - (the first k of a),
       G_k = P_k - d (Hd_k + Tl_k) + (N - k) d^2     ( = sum_t (x_t - m)(x_{t+k} - m) with m = c + d, exactly ),
   and sums over the C chains in a fixed order, without atomics.  The state belongs to the handle, is sized by the run
   (p x C x (2 LT + L + 3) doubles with LT = 8, 32 or 64 the first of them >= L, plus 64 p C draws; at p = 256, C = 65 536,
   L = 31: 13 GB and, fp32, 4 GB), grown by a begin that needs more and kept until cesx_destroy; cesx_set_problem does not
   touch it.  The followed chains are the first C of the [kept][p][J_local] layout. */
#define CESX_CHAIN_ACF_LAGS_MAX 64
/* Clears the stage for a run of N = n_draws draws, L = lags in [1, CESX_CHAIN_ACF_LAGS_MAX] and C = n_chains in
   [1, J_local].  CESX_EINVAL (text in cesx_last_error) outside these, for n_draws < max(4, lags + 2) or for a sharded handle
   (J_local != J_global); the run in hand, if any, then goes on unharmed.  Launches nothing. */
int cesx_chain_acf_begin(cesx_handle h, int n_draws, int lags, int n_chains, void* stream);
/* Adds `kept` draws laid out [kept][p][J_local] in the engine dtype: the arguments of cesx_chain_summary_add.  Reads the
   draws and writes only the stage's own memory (what waits there is read by a later add or by read: the caller's buffer
   is free on return of the launches).  CESX_ESTATE without a begin or past N draws, CESX_EINVAL for a null pointer or
   kept < 1; neither launches anything. */
int cesx_chain_acf_add(cesx_handle h, const void* trace_dev, int kept, void* stream);
/* HOST outputs; synchronises `stream`.  gsum [p][L + 1] = sum over the chains of G_k; msum [p] = sum (m_j - cbar) and
   m2sum [p] = sum (m_j - cbar)^2 about cbar = the mean of the chains' first draws; optional (NULL allowed) chain_gamma
   [L + 1][p][C]: every chain's G_k, and chain_mean [p][C]: every chain's m.  CESX_ESTATE unless exactly N draws were
   added (nothing is launched then), CESX_EINVAL for a null gsum, msum or m2sum; the stage stays readable until the next
   begin. */
int cesx_chain_acf_read(cesx_handle h, double* gsum, double* msum, double* m2sum, double* chain_gamma, double* chain_mean,
                        void* stream);

/* ---- Emulate: GP prediction and the GP sampler over the columns (ces/emulate.py, ces/sample.py:17-119) --
   One exact GP per output, trained on the host (ces_amd/emulate.py); the engine holds its own fp64 image of them and
   evaluates them for every column at once.  GP i maps an input x to z = A_i (x - c) (A_i = diag(1/l_i) S^{-1} lower
   triangular: ARD lengthscales and the enka.scale scaling in one map) and predicts
       mean_i(x) = sum_t alpha_it k_i(z, Z_it) + w_i^T z + b_i,
       var_i(x)  = sigma_i^2 - || L_i^{-1} k_i(z, Z_i.) ||^2   (+ sn_i^2 with the nugget: GPflow's predict_y),
   k_i(z, z') = sigma_i^2 f(|z - z'|), f of family 0 RBF exp(-r^2/2), 1 Matern12, 2 Matern32, 3 Matern52.
   All GP arithmetic is fp64 whatever the engine dtype; the outputs are fp64 (n_gp x J_local) rows.  Sums run in a fixed
   order: runs are bit-reproducible. */
typedef struct {
    uint32_t struct_bytes;    /* sizeof(cesx_gp_desc) */
    int32_t n_gp, J_t;        /* GPs, training points (the input dimension is the handle's p) */
    const double* A;          /* [n_gp][p][p] lower-triangular input maps, row-major */
    const double* c;          /* [p] the input shift */
    const double* Z;          /* [n_gp][J_t][p] the mapped training points */
    const int32_t* family;    /* [n_gp] kernel family 0..3 */
    const double* par;        /* [n_gp][3] sigma^2, sn^2 (likelihood variance), mean bias b */
    const double* mw;         /* [n_gp][p] mean weights w over z */
    const double* alpha;      /* [n_gp][J_t] (K + sn^2 I)^{-1} (y - m(X)) */
    const double* Li;         /* [n_gp][J_t][J_t] L^{-1}, L = chol(K + sn^2 I), row-major (only the lower triangle is read) */
} cesx_gp_desc;
/* Copies the emulator (host fp64) into engine-owned memory; replaces an earlier one. */
int cesx_gp_set(cesx_handle h, const cesx_gp_desc* desc);
/* mean_dev (and var_dev, unless NULL: the mean-only mode) = the n_gp GP rows (fp64, n_gp x J_local) at the columns of X_dev
   (p x J_local, engine dtype); nugget != 0 adds sn^2 to the variance. */
int cesx_gp_predict(cesx_handle h, const void* X_dev, double* mean_dev, double* var_dev, int nugget, void* stream);
/* MCMC.gp_mh over the columns: the proposal is cesx_mh_propose's (cesx_mh_set_proposal with the gp_mh scales; pCN takes the
   same scales), the GP rows of the proposal come from cesx_gp_predict (n_gp == n_obs), and
       phi(u) = 1/2 (m - y)^T Sigma^{-1} (m - y) [+ 1/2 log det Sigma] + 1/2 (u - mu)^T Sigma_prior^{-1} (u - mu)
   with the prior term for RW AND pCN (ces/sample.py:57 / :96), y, mu, Sigma_prior of cesx_set_problem and
       CESX_GP_GAMMA      Sigma = Gamma of cesx_set_problem (mean rows only; a dense Gamma whitened), no log det term
       CESX_GP_VAR        Sigma = diag(var), 1/2 sum log var                (Gamma None; cesx_set_problem's Gamma diagonal)
       CESX_GP_GAMMA_VAR  Sigma = diag(Gamma) + diag(var), 1/2 sum log(..)  (noise_compounded, diagonal Gamma)
   A non-positive variance makes phi NaN (or inf - inf) and the test rejects, as numpy's comparison does.  The start, the
   test, the device uniform, the counters and cesx_mh_stats are those of cesx_mh_start / cesx_mh_accept. */
#define CESX_GP_GAMMA      0
#define CESX_GP_VAR        1
#define CESX_GP_GAMMA_VAR  2
#define CESX_GP_DENSE      3
#define CESX_GP_PROJ       4
int cesx_gp_start(cesx_handle h, int mode, const void* U_dev, const double* mean_dev, const double* var_dev, void* stream);
int cesx_gp_accept(cesx_handle h, int mode, uint64_t step_index, void* U_dev, const void* P_dev, const double* mean_dev,
                   const double* var_dev, const double* logu_dev, void* stream);
/* n_steps Metropolis steps of every chain on the installed emulator in ONE launch (kernels_gpchain.hip, gp_chain_kernel: one
   workgroup per tile of 32 chains), in mode CESX_GP_GAMMA (diagonal or dense Gamma), CESX_GP_VAR or CESX_GP_GAMMA_VAR: per
   step k = 0 .. n_steps - 1 the proposal of cesx_mh_propose, the prediction of cesx_gp_predict (nugget as there; the
   variance only where the mode reads it) and the score and test of cesx_gp_accept, with the noise of step step_index + k --
   xi_dev[n_steps][p][J_local] (engine dtype) and logu_dev[n_steps][J_local] (fp64), or NULL for the device draws of those
   steps: the counter words of cesx_mh_propose / cesx_gp_accept, the normals as an fp64 engine draws them.  The GP rows of
   the proposals stay on chip: for the same fp64 proposal they are bit-identical to cesx_gp_predict's.  Afterwards U_dev, the
   chains' phi, the accept counters and the step count are as n_steps calls of cesx_mh_propose / cesx_gp_predict /
   cesx_gp_accept would have left them (up to the rounding of a different order of the proposal's products): fused launches
   and single steps may alternate, cesx_mh_stats and cesx_mh_phi read the same state.  A proposal whose phi is NaN or
   inf - inf is rejected; a chain whose current phi is NaN stays where it is.
   trace_dev (NULL: none) receives the states after the steps with (k + 1) % stride == 0, laid out [kept][p][J_local] in the
   engine dtype, kept = n_steps / stride.
   All arithmetic inside a launch is fp64 for either engine dtype; an fp32 engine rounds where it stores -- trace_dev, and
   U_dev at the end of the launch: its state is rounded at launch boundaries only, not after every step.
   Limit: a tile's K* panel, GP rows, states and partial sums live in LDS,
       256 (3 p + J_p + 2 n_gp) + 8192 bytes <= 160 KiB,    J_p = J_t rounded up to 16
   (p = 2, n_gp = 10: J_t <= 576); beyond it CESX_EUNSUPPORTED -- the global-memory panel of cesx_gp_predict is not carried
   over, take the step path.
   CESX_ESTATE without cesx_set_problem, cesx_mh_set_proposal, cesx_gp_set or a start (cesx_gp_start / cesx_mh_start);
   CESX_EINVAL for n_steps < 1, stride < 1, a NULL U_dev, a step index that reaches 2^31, mode CESX_GP_DENSE or CESX_GP_PROJ
   (these stay on the step path), a variance mode with a dense Gamma, or n_gp != n_obs.  None of these launches anything. */
int cesx_gp_run(cesx_handle h, int mode, uint64_t step_index, int n_steps, int stride, int nugget, void* U_dev,
                void* trace_dev, const void* xi_dev, const double* logu_dev, void* stream);
/* cesx_gp_predict with the gradients of every GP row with respect to the input x (kernels_gpgrad.hip, gp_grad_kernel: the
   tile of cesx_gp_predict -- one workgroup per (GP, 32 chains), W = L^{-1} k* on v_mfma_f64_16x16x4_f64 -- then a second
   product beta = L^{-T} W from the same packed L^{-1} image read transposed; K^{-1} is never formed).  With h(r) = f'(r) / r
   (RBF -exp(-r^2/2), Matern32 -3 exp(-sqrt(3) r), Matern52 -(5/3)(1 + sqrt(5) r) exp(-sqrt(5) r): finite at r = 0):
       dk_t / dz  = sigma_i^2 h(r_t) (z - Z_it)
       grad_z mean_i = sum_t alpha_it dk_t / dz + w_i,   grad_z var_i = -2 sum_t beta_t dk_t / dz,   grad_x = A_i^T grad_z
   (the nugget adds nothing to a gradient).  mean_dev and var_dev as cesx_gp_predict writes them, BIT FOR BIT; dmean_dev and
   dvar_dev fp64 [n_gp][p][J_local].  var_dev and dvar_dev both NULL is the mean-only mode: no triangular product; one of them
   NULL alone is CESX_EINVAL.  The sums run on the vector ALU in a fixed order, no atomics: runs are bit-reproducible.
   A tile keeps z, both z-gradients and two J_p x 32 panels (K* then beta, W): (2 J_p + 3 p) 256 bytes next to the 8 KiB of
   partial sums (J_p + 3 p in the mean-only mode).  Up to 2 J_p + 3 p <= 608 that is LDS; beyond it the tiles live in the
   global workspace of cesx_gp_predict, one slot per workgroup, and the (GP, tile) pairs go in as many launches of `stream`
   as the slots need: every J_t that cesx_gp_predict takes works.
   CESX_ESTATE without cesx_gp_set; CESX_EUNSUPPORTED for an emulator with a Matern12 GP (no gradient at a training point).
   Neither launches anything. */
int cesx_gp_predict_grad(cesx_handle h, const void* X_dev, double* mean_dev, double* var_dev, double* dmean_dev,
                         double* dvar_dev, int nugget, void* stream);
/* MCMC.gp_mh(chains=M, update='langevin'): a preconditioned Metropolis-adjusted Langevin step on the emulated posterior, every
   column a chain, on the step path.  Proposal kind CESX_MH_LANGEVIN (cesx_mh_set_proposal): S the lower-triangular scale of
   the random walk, so the caller's delta is the Langevin step.  With phi as for cesx_gp_start in mode CESX_GP_GAMMA, _VAR or
   _GAMMA_VAR, d = mean - y and
       grad phi(u) = sum_i (a_i grad mean_i + b_i grad var_i) + Sigma_prior^{-1} (u - mu)
       CESX_GP_GAMMA, diagonal Gamma      a_i = d_i / Gamma_ii,  b = 0
       CESX_GP_GAMMA, dense Gamma         a = L_Gamma^{-T} (L_Gamma^{-1} mean - y~),  b = 0
       CESX_GP_VAR, CESX_GP_GAMMA_VAR     a_i = d_i / v_i,  b_i = 1/2 (1 / v_i - d_i^2 / v_i^2),  v_i = var_i (+ Gamma_ii)
   g(u) = S^T grad phi(u) and xi ~ N(0, I):
       cesx_gp_langevin_start     phi(U) and g(U) from the rows and gradients of cesx_gp_predict_grad at U; counters cleared
       cesx_gp_langevin_propose   P = U + S (xi - g(U) / 2)       (xi_dev the injected block, engine dtype, or NULL: the device
                                  draw of cesx_mh_propose for step_index; either way the block is kept in engine memory)
       cesx_gp_langevin_accept    phi(P), g(P) from the rows and gradients at P, then the test
                                      log u < phi(U) - phi(P) + 1/2 |xi|^2 - 1/2 |xi - (g(U) + g(P)) / 2|^2
                                  with the block the last propose kept (no S^{-1}: S^{-1} (P - U + S S^T grad phi(U) / 2) = xi by
                                  construction) and cesx_gp_accept's log u; accepted columns: U := P, phi := phi(P), g := g(P),
                                  counter + 1.  The caller passes the same step_index to propose and accept.
   A NaN or inf - inf in phi(P), g(P) or the correction rejects; a chain whose own phi or g is NaN stays where it is.  One
   thread per chain (kernels_gpgrad.hip, lv_*), fp64, fixed orders: bit-reproducible.  The counters, cesx_mh_stats and
   cesx_mh_phi are those of cesx_gp_start / cesx_gp_accept.  var_dev and dvar_dev may be NULL in mode CESX_GP_GAMMA.
   CESX_ESTATE without cesx_set_problem, a proposal of kind CESX_MH_LANGEVIN, cesx_gp_set or (propose, accept) a
   cesx_gp_langevin_start; accept also without a propose since the start or the last accept.  CESX_EINVAL for mode
   CESX_GP_DENSE or CESX_GP_PROJ, an unknown mode, a variance mode with a dense Gamma, n_gp != n_obs, a null pointer, P_dev
   aliasing U_dev or a step index >= 2^31.  None of these launches anything or touches U_dev or the chains' phi. */
int cesx_gp_langevin_start(cesx_handle h, int mode, const void* U_dev, const double* mean_dev, const double* var_dev,
                           const double* dmean_dev, const double* dvar_dev, void* stream);
int cesx_gp_langevin_propose(cesx_handle h, uint64_t step_index, const void* U_dev, const void* xi_dev, void* P_dev, void* stream);
int cesx_gp_langevin_accept(cesx_handle h, int mode, uint64_t step_index, void* U_dev, const void* P_dev, const double* mean_dev,
                            const double* var_dev, const double* dmean_dev, const double* dvar_dev, const double* logu_dev,
                            void* stream);
/* CESX_GP_DENSE: k GPs on PCA-decorrelated outputs (pca_tools of ces/emulate.py:74-77 and ces/sample.py:52-53, :91-92).  The
   data space is rebuilt per chain j from column j of the (k x J_local) rows of cesx_gp_predict (n_gp == k):
       d = B m_j + g0 - y,    Sigma_j = Gamma + B diag(v_j) B^T,    phi = 1/2 d^T Sigma_j^{-1} d [+ 1/2 log det Sigma_j] + prior term
   with y and Gamma of cesx_set_problem as given (dense or diagonal; NOT whitened) and the prior term of the other modes.
   Sigma_j is a dense n x n matrix per chain and state: one wave factors it (Cholesky, resident in LDS) and scores, all in
   fp64 in one fixed order -- two calls are bit-identical and a chain's phi does not depend on J_local, on its column or on
   its neighbours.  A pivot that is not > 0 or not finite makes phi NaN: the test rejects, a start state stays stuck.
   Limits: 1 <= k <= n_obs <= CESX_GP_DENSE_NMAX. */
#define CESX_GP_DENSE_NMAX 128
typedef struct {
    uint32_t struct_bytes;    /* sizeof(cesx_gp_dense_desc) */
    int32_t k;                /* columns of B = GPs */
    int32_t logdet;           /* != 0: add 1/2 log det Sigma_j (noise_compounded, ces/sample.py:69-72) */
    const double* B;          /* [n][k] row-major (VD_k) */
    const double* g0;         /* [n] (mG) or NULL = 0 */
} cesx_gp_dense_desc;
/* Copies the descriptor (host fp64); replaces an earlier one.  CESX_EINVAL (text in cesx_last_error) for k < 1, k > n_obs,
   n_obs > CESX_GP_DENSE_NMAX or a null B -- the installed descriptor stays; CESX_ESTATE without a problem.  A later
   cesx_set_problem drops the descriptor, as it drops the proposal.  cesx_gp_start / cesx_gp_accept in mode CESX_GP_DENSE
   return CESX_ESTATE without one, and need var_dev and n_gp == k. */
int cesx_gp_dense_set(cesx_handle h, const cesx_gp_dense_desc* desc);
/* CESX_GP_PROJ: the likelihood of CESX_GP_DENSE with Sigma_j projected to k x k, for any n_obs.  With Gamma = L L^T,
   W = L^{-1} B = Q R (thin QR, R k x k upper triangular) and r0 = L^{-1} (g0 - y):
       Sigma_j = L (I_n + Q S_j Q^T) L^T,  S_j = R diag(v_j) R^T,   a_j = a0 + R m_j,  a0 = Q^T r0,  c_perp = |(I - Q Q^T) r0|^2
       d^T Sigma_j^{-1} d = c_perp + a_j^T (I_k + S_j)^{-1} a_j,      log det Sigma_j = 2 sum log diag(L) + log det (I_k + S_j)
   I_k + S_j has eigenvalues >= 1 and every term of the quadratic form is a sum of squares: nothing cancels, however large
   B diag(v) B^T is beside Gamma.  The caller reduces the problem once on the host (ces_amd.emulate.project_sigma) and hands
   R, a0 and the two scalars over; y and Gamma of cesx_set_problem are NOT read in this mode (they are baked into the
   descriptor), and n_obs carries no limit.  Per chain one sub-wave group of lanes factors I_k + S_j (Cholesky, resident
   in LDS) and scores, all in fp64 in one fixed order -- two calls are bit-identical and a chain's phi does not depend on
   J_local, on its column, on its place in the wave or on its neighbours.  A pivot that is not > 0 or not finite makes phi
   NaN: the test rejects, a start state stays stuck.  Limits: 1 <= k <= CESX_GP_PROJ_KMAX. */
#define CESX_GP_PROJ_KMAX 128
typedef struct {
    uint32_t struct_bytes;    /* sizeof(cesx_gp_proj_desc) */
    int32_t k;                /* GPs = the order of R */
    int32_t logdet;           /* != 0: add half_logdet_gamma + 1/2 log det (I_k + S_j) (noise_compounded) */
    const double* R;          /* [k][k] row-major; only the upper triangle is read */
    const double* a0;         /* [k] */
    double c_perp;            /* >= 0 */
    double half_logdet_gamma; /* sum log diag(L) = 1/2 log det Gamma */
} cesx_gp_proj_desc;
/* Copies the descriptor (host fp64); replaces an earlier one.  CESX_EINVAL (text in cesx_last_error) for k < 1,
   k > CESX_GP_PROJ_KMAX, a null pointer, a non-finite entry or c_perp < 0 -- the installed descriptor stays; CESX_ESTATE
   without a problem.  A later cesx_set_problem drops the descriptor.  cesx_gp_start / cesx_gp_accept in mode CESX_GP_PROJ
   return CESX_ESTATE without one, and need var_dev and n_gp == k. */
int cesx_gp_proj_set(cesx_handle h, const cesx_gp_proj_desc* desc);
/* The gradient samplers on the projected Sigma: MCMC.gp_mh(chains=M, pca_tools=, sigma_form='projected', update='langevin' /
   'hmc').  Per chain, with a = a0 + R m, A = I_k + R diag(v) R^T = L L^T and z = L^{-1} a (the factor of CESX_GP_PROJ above):
       phi_data = 1/2 (c_perp + |z|^2) [+ half_logdet_gamma + sum log L_cc]        (the data term of cesx_gp_start's phi, its bits)
       w   = L^{-T} z = A^{-1} a
       e_t = (R^T w)_t = d phi / d m_t                       ( = B_t^T Sigma^{-1} d in the data space )
       h_t = |L^{-1} R[:, t]|^2 = (R^T A^{-1} R)_tt          ( = B_t^T Sigma^{-1} B_t )
       a_t = e_t,   b_t = 1/2 ([logdet] h_t - e_t^2) = d phi / d v_t
       grad phi = sum_t (a_t grad m_t + b_t grad v_t) + Sigma_prior^{-1} (u - mu)
   (without the descriptor's logdet flag the h term is absent: the gradient is the gradient of the phi that is scored).  With
   R = I and a diagonal Gamma this is the variance mode of cesx_gp_langevin_*.  One launch (kernels_gpprojgrad.hip) on the
   placement of the score launch -- a sub-wave group of lanes per chain, the factor resident in LDS -- forms phi_data, a and
   b, all in fp64 in one fixed order: bit-reproducible, independent of J_local, of the column and of the neighbours; a pivot
   that is not > 0 or not finite makes phi_data, a and b of that chain NaN (a proposal into it is rejected, a start state in
   it stays stuck).  The lv_* / hm_* kernels then form the prior term, grad phi and g = S^T grad phi as in the other modes.
       cesx_gp_proj_coef            the coefficient launch alone, from the (k x J_local) rows into caller buffers: phi_dev
                                    [J_local], a_dev and b_dev [k][J_local], fp64
       cesx_gp_proj_langevin_start / cesx_gp_proj_langevin_accept, cesx_gp_proj_hmc_leap / cesx_gp_proj_hmc_accept
                                    cesx_gp_langevin_start / _accept and cesx_gp_hmc_leap / _accept without `mode`: the rows
                                    and gradients (k x J_local, k x p x J_local) of cesx_gp_predict_grad.  The proposal and the
                                    begin of a trajectory are cesx_gp_langevin_propose and cesx_mh_hmc_begin, which take no
                                    mode; steps of both families alternate on one handle, and an armed handle
                                    (cesx_mh_adapt_set) adapts through the hmc pair as through cesx_gp_hmc_*.
   The cesx_gp_langevin_* and cesx_gp_hmc_* calls keep answering CESX_EINVAL for CESX_GP_DENSE and CESX_GP_PROJ.
   CESX_ESTATE without a descriptor (cesx_gp_proj_set) or cesx_gp_set, and in the sequencing states of the namesakes;
   CESX_EUNSUPPORTED for an emulator with a Matern12 GP; CESX_EINVAL for n_gp != k, a null pointer (var_dev and dvar_dev are
   needed), P_dev / Q_dev aliasing U_dev or a step index >= 2^31.  None of these launches anything. */
int cesx_gp_proj_coef(cesx_handle h, const double* mean_dev, const double* var_dev, double* phi_dev, double* a_dev, double* b_dev,
                      void* stream);
int cesx_gp_proj_langevin_start(cesx_handle h, const void* U_dev, const double* mean_dev, const double* var_dev,
                                const double* dmean_dev, const double* dvar_dev, void* stream);
int cesx_gp_proj_langevin_accept(cesx_handle h, uint64_t step_index, void* U_dev, const void* P_dev, const double* mean_dev,
                                 const double* var_dev, const double* dmean_dev, const double* dvar_dev, const double* logu_dev,
                                 void* stream);
int cesx_gp_proj_hmc_leap(cesx_handle h, void* Q_dev, const double* mean_dev, const double* var_dev, const double* dmean_dev,
                          const double* dvar_dev, void* stream);
int cesx_gp_proj_hmc_accept(cesx_handle h, uint64_t step_index, void* U_dev, const void* Q_dev, const double* mean_dev,
                            const double* var_dev, const double* dmean_dev, const double* dvar_dev, const double* logu_dev,
                            void* stream);

/* ---- Emulate: training the GPs on device (ces_amd/emulate.py train_gps(device=True)) --------------------
   The log marginal likelihood of n_gp exact GPs on SHARED training inputs X and its gradient, all GPs of a call in the same
   launches (their number depends on J_t, not on n_gp).  GP i has the natural parameters, in GPR._get() order,
       theta_i = (sigma^2, l_1..l_p (ard != 0) or one l, sn^2, then the mean's: none / c / A_1..A_p, b),
   Ky = sigma^2 f(|x_a / l - x_b / l|) + sn^2 I (f of `family` as for cesx_gp_set; r from direct differences of the scaled
   inputs, 0 on the diagonal), L = chol(Ky), alpha = L^{-T} L^{-1} (y_i - m(X)),
       lml = -1/2 r^T alpha - sum log L_aa - 1/2 J_t log 2 pi,     d lml / d theta as GPR.log_marginal_likelihood_and_grad().
   All arithmetic fp64 whatever the engine dtype; every sum runs in a fixed order: two calls are bit-identical.  The
   positive transform of the optimiser stays with the caller. */
#define CESX_GPFIT_MEAN_ZERO      0
#define CESX_GPFIT_MEAN_CONSTANT  1
#define CESX_GPFIT_MEAN_LINEAR    2
typedef struct {
    uint32_t struct_bytes;    /* sizeof(cesx_gpfit_desc) */
    int32_t n_gp, J_t;        /* GPs, training points (the input dimension is the handle's p) */
    int32_t family;           /* kernel family 0..3, one for the whole problem */
    int32_t ard;              /* != 0: p lengthscales per GP, else one */
    int32_t mean;             /* CESX_GPFIT_MEAN_* */
    const double* X;          /* [J_t][p] training inputs, row-major */
    const double* Y;          /* [n_gp][J_t] targets */
} cesx_gpfit_desc;
/* Copies the problem (host fp64) and allocates ALL the workspace of an evaluation (per GP three J_t^2 fp64 images: L,
   L^{-T}, K^{-1}, padded to a multiple of 16; cesx_gpfit_eval allocates nothing).  Replaces an earlier fit problem; a call
   that fails (a bad argument included) leaves the handle WITHOUT one and frees what it had allocated. */
int cesx_gpfit_set(cesx_handle h, const cesx_gpfit_desc* desc);
/* Parameters per GP of the installed fit problem (-1: none). */
int cesx_gpfit_ntheta(cesx_handle h);
/* The GPs idx[0 .. n_active) (distinct) at theta [n_active][n_theta]: lml [n_active], grad [n_active][n_theta] and
   status [n_active] = CESX_OK or CESX_ENOTPD (a pivot of that GP's factorisation was not > 0: its lml and grad mean nothing,
   the other GPs of the call are unaffected).  Host pointers; synchronises `stream`. */
int cesx_gpfit_eval(cesx_handle h, int n_active, const int32_t* idx, const double* theta, double* lml, double* grad,
                    int32_t* status, void* stream);
/* alpha [J_t] and L^{-1} [J_t][J_t] (row-major, zero above the diagonal: what cesx_gp_desc takes) of GP i AS OF ITS LAST
   EVALUATION, to the host.  Synchronises. */
int cesx_gpfit_factors(cesx_handle h, int i, double* alpha, double* Li);

/* ---- host staging ------------------------------------------------------ */

/* A COLUMN block of a row-major (rows, J) ensemble between pinned host memory and the device, asynchronously on
   `stream` (hipMemcpy2DAsync; pitches and width in bytes, `height` rows, to_device != 0: host -> device).  The
   drop-in class pipelines the reference's host data flow (ces/calibrate.py:341-369: G_ens on the host, arrays into
   and out of every update) over such blocks: particles are independent in G_ens (:123-130), rows are not. */
int cesx_copy_cols_async(cesx_handle h, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes,
                      size_t height, int to_device, void* stream);

/* ---- introspection ---------------------------------------------------- */

/* Per-kernel timing with HIP events recorded on the launch stream around the
   two O(J) kernels (which: 0 = Gram/moments kernel K1, 1 = update kernel K3).
   cesx_profile_read synchronises, returns the summed milliseconds and the
   number of launches since the last read, and resets the counters. */
/* on = 2: "gap-only" -- only the stop of the second moments launch and the start of the update launch are bound
   (for cesx_profile_gap); such a step contributes nothing to cesx_profile_read.
   on = 3 / 4: only the update / only the moments launches carry events (a time-stamped dispatch costs the step
   20-30 us: a timed region samples its dominant kernel alone). */
int cesx_profile_enable(cesx_handle h, int on);
int cesx_profile_read(cesx_handle h, int which, double* total_ms, int* launches);
/* Milliseconds from the end of the last profiled moments launch to the start of the last profiled update launch
   (the K2 kernels, the hand-over from the side stream and -- sharded -- the collectives sit in between): call it
   after the profiled step and BEFORE cesx_profile_read, which recycles the events.  -1 when nothing was profiled. */
int cesx_profile_gap(cesx_handle h, double* gap_ms);
/* Shader clock (GHz) the last PROFILED update launch (K3) ran at: one wave of it stamps s_memtime and the 100 MHz
   s_memrealtime at its start and end (profiled launches only; the others execute no stamp).  Synchronises.
   0.0 when no profiled launch has run. */
int cesx_profile_clock(cesx_handle h, double* clock_ghz);
/* What this device sustains on the bare matrix instruction of the engine's dtype (v_mfma_f32_32x32x2_f32 /
   v_mfma_f64_16x16x4_f64, operands in registers, every SIMD busy) for about target_ms milliseconds: TFLOP/s
   and the in-kernel shader clock.  A roofline fraction can then be read against the datasheet peak and against
   this box's own rate.  Measurement support only; synchronises. */
int cesx_calibrate_mfma(cesx_handle h, double target_ms, double* tflops, double* clock_ghz, void* stream);

/* Host-only introspection for tests: the work partition of the moments launch `part` (0: U x U blocks, 1: the
   others) for a handle of this shape and workgroup budget, checked for its invariants (every wanted block of the
   lower triangle exactly once, slices x whole tiles cover J, staged rows fit in LDS, workgroups within the budget).
   Returns the number of violations (0 = sound), < 0 on bad arguments; info[6] (optional) = {types, workgroups,
   blocks, busiest workgroup's tiles x blocks per SIMD, max staged row blocks, slabs}.  Needs no device. */
int cesx_debug_gram_plan(int p, int n_obs, int dtype, int part, int wg_budget, long long J_local, int* info);

/* Host-only introspection for tests: the K2 (dense algebra) the library runs for an engine state and a launch, both
   given as facts[23] = {update, time_step, phase (0 step, 1 aldi_constant drift, 2 aldi_constant noise), an update
   kernel takes the hk-free image, dtype, potrf_ld(p) <= 256, diagonal Sigma, chained image; hk-free allowed, LDS-DMA
   update kernels, the image is allocated; of the last cesx_chol_async: in flight, centring fused into its load, L
   into the image, signals, d_L left out; polled join allowed, sharded, the caller is on the side stream, the caller's
   stream has a lower priority than the side stream; CESX_FUSE_CENTER=1, no CESX_FUSE_CENTER given, short second Gram
   launch}.  plan[13] = {route (0 noise only, 1 tail, 2 finish, 3 general), tail arm (1 dense Sigma, 2 chained,
   3 plain), join of the side stream (0 none, 1 event, 2 polled), U part (0 side stream, 1 centring launch, 2 fused
   into the factorisation's load), centring parts (1 U | 2 G | 4 keep the status word), in-line factorisation (1 image,
   2 fp64), re-factorisation of an image-only factor, M = C Sigma^{-1} GEMM, spectral block, gain inverse, EKS inverse,
   assemble mode (0 aldi, 1 eks, 2 constant drift, 3 constant noise), its ktot for kp = 16, kn = 32, ktot = 64 (0: no
   assemble launch)}.  Returns 0, < 0 on bad arguments.  Needs no handle and no device. */
int cesx_debug_dense_plan(const int32_t* facts, int32_t* plan);

/* Copies the engine's current small dense state to HOST buffers (any may be
   NULL): ubar (p), gbar (n), C (p x p), L = chol(C) (p x p), K (p x n),
   M = C Sigma^{-1} (p x p).  Synchronises.  After a step that kept L in its coefficient image only
   (cesx_debug_update_form 2), L is factored again from the C the engine holds now. */
int cesx_debug_dense(cesx_handle h, double* ubar, double* gbar, double* C, double* L,
                     double* K, double* M);

#ifdef __cplusplus
}
#endif
#endif /* CESX_H */
