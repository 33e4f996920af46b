"""ctypes binding of ``libcesx.so`` (include/cesx.h).

PyTorch-ROCm tensors are used only as device buffers and for the current HIP
stream; every number is produced by the hand-written HIP kernels behind the C
ABI.  There is no CPU fallback: if the library is missing or no GPU is
present the product path raises.
"""
import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CESX_LIB") or os.path.join(_HERE, "libcesx.so")      # (CESX_LIB: a dev build of the same ABI)

OK, EINVAL, ENOTPD, EHIP, ESTATE, EUNSUPPORTED, ENOCONV = 0, 1, 2, 3, 4, 5, 6
F32, F64 = 0, 1
UPDATES = {"eks": 0, "aldi": 1, "aldi_constant": 2}
TIME_STEPS = {None: 0, "spectral": 1, "constant": 2, "adaptive": 3, "mix": 4}
ABI_VERSION = 10
MH_KINDS = {None: 0, "pCN": 1, "langevin": 2, "hmc": 2}     # ('hmc' runs under the Langevin proposal: cesx_mh_hmc_*) kwargs['update'] of MCMC.model_mh (ces/sample.py:165-168) -> CESX_MH_RW / CESX_MH_PCN; build-only: CESX_MH_LANGEVIN (gp_mh and model_mh)

EXPORTS = ("cesx_abi_version", "cesx_create", "cesx_destroy", "cesx_last_error", "cesx_set_problem",
           "cesx_step", "cesx_result", "cesx_moments_len", "cesx_colsum", "cesx_set_shift",
           "cesx_moments", "cesx_apply", "cesx_apply_drift", "cesx_apply_finish", "cesx_draw_noise",
           "cesx_forward_lineal", "cesx_debug_dense", "cesx_profile_enable", "cesx_profile_read",
           "cesx_moments_uu_len", "cesx_moments_uu", "cesx_chol_async", "cesx_moments_rest", "cesx_side_stream",
           "cesx_prefetch_noise", "cesx_forward_set_lineal", "cesx_forward_apply", "cesx_moments_uu_chol", "cesx_debug_poll_recoveries", "cesx_comm_unique_id", "cesx_comm_init", "cesx_comm_destroy", "cesx_comm_nranks",
           "cesx_comm_stats", "cesx_allreduce_head", "cesx_allreduce_tail", "cesx_allreduce_whole", "cesx_allreduce_sum", "cesx_allreduce_max", "cesx_moments_uu_handover", "cesx_debug_gram_plan", "cesx_debug_dense_plan",
           "cesx_profile_clock", "cesx_calibrate_mfma", "cesx_profile_gap", "cesx_moments_rest_lineal", "cesx_copy_cols_async",
           "cesx_debug_warm_inverse", "cesx_debug_update_form", "cesx_comm_count",
           "cesx_mh_set_proposal", "cesx_mh_start", "cesx_mh_propose", "cesx_mh_accept", "cesx_mh_stats", "cesx_mh_phi",
           "cesx_gp_set", "cesx_gp_predict", "cesx_gp_start", "cesx_gp_accept", "cesx_gp_run", "cesx_gp_dense_set", "cesx_gp_proj_set",
           "cesx_gp_predict_grad", "cesx_gp_langevin_start", "cesx_gp_langevin_propose", "cesx_gp_langevin_accept",
           "cesx_gp_proj_coef", "cesx_gp_proj_langevin_start", "cesx_gp_proj_langevin_accept", "cesx_gp_proj_hmc_leap", "cesx_gp_proj_hmc_accept",
           "cesx_gpfit_set", "cesx_gpfit_ntheta", "cesx_gpfit_eval", "cesx_gpfit_factors",
           "cesx_darcy_set", "cesx_darcy_apply", "cesx_darcy_set_streamed", "cesx_darcy_workspace_bytes", "cesx_lorenz_set", "cesx_lorenz_apply",
           "cesx_darcy_grad", "cesx_darcy_grad_lds_bytes",
           "cesx_lorenz_three_set", "cesx_lorenz_three_apply", "cesx_map_set", "cesx_map_apply", "cesx_mh_run_map",
           "cesx_map_jac", "cesx_mh_langevin_start", "cesx_mh_langevin_propose", "cesx_mh_langevin_accept", "cesx_mh_langevin_run_map",
           "cesx_mh_langevin_lineal_set", "cesx_mh_langevin_lineal_start", "cesx_mh_langevin_lineal_propose",
           "cesx_mh_langevin_lineal_accept", "cesx_mh_langevin_lineal_g",
           "cesx_mh_hmc_lineal_begin", "cesx_mh_hmc_lineal_leap", "cesx_mh_hmc_lineal_accept",
           "cesx_mh_hmc_begin", "cesx_mh_hmc_leap", "cesx_mh_hmc_accept", "cesx_gp_hmc_leap", "cesx_gp_hmc_accept", "cesx_mh_hmc_run_map",
           "cesx_mh_adapt_set", "cesx_mh_adapt_read", "cesx_mh_grad_source",
           "cesx_chain_summary_begin", "cesx_chain_summary_add", "cesx_chain_summary_read",
           "cesx_chain_hist_begin", "cesx_chain_hist_add", "cesx_chain_hist_read",
           "cesx_chain_acf_begin", "cesx_chain_acf_add", "cesx_chain_acf_read")
L96_STATUS = {1: "the step size fell below the spacing between numbers (scipy's step-size failure)",
              2: "a state or an error norm was not finite",
              3: "max_attempts steps were attempted"}
L63_STATUS = L96_STATUS                # cesx_lorenz_three_apply reports a particle as cesx_lorenz_apply does
GPFIT_MEANS = {"zero": 0, "constant": 1, "linear": 2}   # CESX_GPFIT_MEAN_*
GP_MODES = {"gamma": 0, "var": 1, "gamma_var": 2, "dense": 3, "proj": 4}     # CESX_GP_GAMMA / _VAR / _GAMMA_VAR / _DENSE / _PROJ: Sigma of MCMC.gp_mh (ces/sample.py:48-55)
GP_DENSE_NMAX = 128                                   # CESX_GP_DENSE_NMAX
GP_PROJ_KMAX = 128                                    # CESX_GP_PROJ_KMAX
GRAD_SOURCES = {"jacobian": 0, "ready": 1}            # CESX_MH_GRAD_JACOBIAN / _READY (cesx_mh_grad_source)
MAP_KINDS = {"elliptic": 1, "banana": 2, "exp": 3}    # CESX_MAP_ELLIPTIC / _BANANA / _EXP (ces_amd.utils elliptic, banana, lineal_log)
MAP_FUSED = ("elliptic", "banana")                    # the kinds cesx_mh_run_map has a kernel for


class Config(C.Structure):
    _fields_ = [("struct_bytes", C.c_uint32), ("p", C.c_int32), ("n_obs", C.c_int32), ("dtype", C.c_int32),
                ("device", C.c_int32), ("J_local", C.c_int64), ("J_global", C.c_int64),
                ("j_offset", C.c_int64), ("seed", C.c_uint64)]


class StepParams(C.Structure):
    _fields_ = [("struct_bytes", C.c_uint32), ("update", C.c_int32), ("time_step", C.c_int32),
                ("first_step", C.c_int32), ("t_len", C.c_int32), ("reserved", C.c_int32),
                ("t_last", C.c_double), ("delta_t", C.c_double), ("spinup", C.c_double),
                ("switch_mult", C.c_double), ("step_index", C.c_uint64)]


class StepResult(C.Structure):
    _fields_ = [("hk", C.c_double), ("t_new", C.c_double), ("self_bias", C.c_double),
                ("self_bias_data", C.c_double), ("bias_data", C.c_double), ("bias", C.c_double),
                ("radspec", C.c_double), ("lag_bias_data", C.c_double), ("lag_self_bias_data", C.c_double),
                ("status", C.c_int32), ("reserved", C.c_int32)]


class GpDesc(C.Structure):
    _fields_ = [("struct_bytes", C.c_uint32), ("n_gp", C.c_int32), ("J_t", C.c_int32),
                ("A", C.c_void_p), ("c", C.c_void_p), ("Z", C.c_void_p), ("family", C.c_void_p),
                ("par", C.c_void_p), ("mw", C.c_void_p), ("alpha", C.c_void_p), ("Li", C.c_void_p)]


class GpDenseDesc(C.Structure):
    _fields_ = [("struct_bytes", C.c_uint32), ("k", C.c_int32), ("logdet", C.c_int32), ("B", C.c_void_p), ("g0", C.c_void_p)]


class GpProjDesc(C.Structure):
    _fields_ = [("struct_bytes", C.c_uint32), ("k", C.c_int32), ("logdet", C.c_int32), ("R", C.c_void_p), ("a0", C.c_void_p),
                ("c_perp", C.c_double), ("half_logdet_gamma", C.c_double)]


class GpFitDesc(C.Structure):
    _fields_ = [("struct_bytes", C.c_uint32), ("n_gp", C.c_int32), ("J_t", C.c_int32), ("family", C.c_int32),
                ("ard", C.c_int32), ("mean", C.c_int32), ("X", C.c_void_p), ("Y", C.c_void_p)]


class DarcyDesc(C.Structure):
    _fields_ = [("struct_bytes", C.c_uint32), ("K", C.c_int32), ("p", C.c_int32), ("n_obs", C.c_int32),
                ("coef", C.c_void_p), ("scatter", C.c_void_p), ("D", C.c_void_p), ("S", C.c_void_p), ("R", C.c_void_p),
                ("obs_index", C.c_void_p)]


class L96Desc(C.Structure):
    _fields_ = [("struct_bytes", C.c_uint32), ("n_slow", C.c_int32), ("n_fast", C.c_int32), ("n_obs", C.c_int32),
                ("p", C.c_int32), ("stat_mode", C.c_int32), ("par_row", C.c_int32 * 4), ("par_fixed", C.c_double * 4),
                ("T", C.c_double), ("max_step", C.c_double), ("rtol", C.c_double), ("atol", C.c_double),
                ("n_t", C.c_int32), ("t", C.c_void_p), ("spinup_samples", C.c_int32), ("window_samples", C.c_int32),
                ("max_attempts", C.c_int64)]


def l96_desc_struct(desc):
    """``desc`` (the dict ``ces_amd.models.lorenz96.device_descriptor`` returns) as a cesx_l96_desc, and the array its ``t``
    points into (keep it alive for the call)."""
    t = np.ascontiguousarray(np.asarray(desc["t"], dtype=np.float64).reshape(-1))
    d = L96Desc()
    d.struct_bytes = C.sizeof(L96Desc)
    d.n_slow, d.n_fast, d.n_obs, d.p = int(desc["n_slow"]), int(desc["n_fast"]), int(desc["n_obs"]), int(desc["p"])
    d.stat_mode = int(desc["stat_mode"])
    for k in range(4):
        d.par_row[k] = int(desc["par_row"][k])
        d.par_fixed[k] = float(desc["par_fixed"][k])
    d.T, d.max_step, d.rtol, d.atol = float(desc["T"]), float(desc["max_step"]), float(desc["rtol"]), float(desc["atol"])
    d.n_t, d.t = t.size, t.ctypes.data
    d.spinup_samples, d.window_samples = int(desc["spinup_samples"]), int(desc["window_samples"])
    d.max_attempts = int(desc.get("max_attempts", 1000000))
    return d, t


class L63Desc(C.Structure):
    _fields_ = [("struct_bytes", C.c_uint32), ("par_row", C.c_int32 * 3), ("par_fixed", C.c_double * 3),
                ("par_log", C.c_int32 * 3), ("t0", C.c_double), ("T", C.c_double), ("max_step", C.c_double),
                ("rtol", C.c_double), ("atol", C.c_double), ("n_t", C.c_int32), ("t", C.c_void_p),
                ("window_samples", C.c_int32), ("max_attempts", C.c_int64)]


def l63_desc_struct(desc):
    """``desc`` (the dict ``ces_amd.models.lorenz63.device_descriptor`` returns) as a cesx_l63_desc, and the array its ``t``
    points into (keep it alive for the call)."""
    t = np.ascontiguousarray(np.asarray(desc["t"], dtype=np.float64).reshape(-1))
    d = L63Desc()
    d.struct_bytes = C.sizeof(L63Desc)
    for k in range(3):
        d.par_row[k] = int(desc["par_row"][k])
        d.par_fixed[k] = float(desc["par_fixed"][k])
        d.par_log[k] = int(desc["par_log"][k])
    d.t0, d.T = float(desc["t0"]), float(desc["T"])
    d.max_step, d.rtol, d.atol = float(desc["max_step"]), float(desc["rtol"]), float(desc["atol"])
    d.n_t, d.t = t.size, t.ctypes.data
    d.window_samples = int(desc["window_samples"])
    d.max_attempts = int(desc.get("max_attempts", 1000000))
    return d, t


class MapDesc(C.Structure):
    _fields_ = [("struct_bytes", C.c_int), ("kind", C.c_int), ("prm", C.c_double * 8)]


class ChainHistDesc(C.Structure):
    _fields_ = [("struct_bytes", C.c_uint32), ("bins", C.c_int32), ("bins2d", C.c_int32), ("n_pairs", C.c_int32),
                ("edges1", C.c_void_p), ("edges2", C.c_void_p), ("pairs", C.c_void_p)]


class CesxError(RuntimeError):
    def __init__(self, code, msg, result=None):
        super().__init__("cesx error %d: %s" % (code, msg))
        self.code = code
        self.result = result      # cesx_result's CESX_ESTATE after a re-run step: the (valid) result of that step


_lib = None


def cpu_share():
    """Host cores this process may actually use: the cgroup CPU quota when there is one (a GPU box exposes 256
    logical CPUs and gives a one-GPU job a 16-core share), else the affinity mask."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, q // per))
        except (OSError, ValueError, IndexError):
            pass
    return n


def default_copy_threads():
    """Host threads for the staging casts.  They are memory-bound (4 threads already move a 256 x 65 536 block in
    1.5 ms) and they run right after the caller's own BLAS threads, which keep spinning for a while: on a box with
    a cgroup CPU quota the two pools TOGETHER must stay within the quota, or the kernel throttles the whole process
    for the rest of the 100-ms period -- 40-50 ms stalls in whatever phase runs next (round 3, tools/hostloop_probe.py:
    16 BLAS + 16 copy threads on a 16-core share: every period throttled, 30.7 ms per iteration; 12 + 4: none, 18.5).
    A quarter of the share, at least 2, at most 8 (CESX_COPY_THREADS overrides)."""
    env = os.environ.get("CESX_COPY_THREADS")
    if env:
        return max(1, int(env))
    return max(2, min(8, cpu_share() // 4))


def load_library(path=None):
    """Load libcesx.so and declare its prototypes.  Loud failure when absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise ImportError("%s not found: build it with `python -m ces_amd.build` "
                          "(there is no CPU fallback for the HIP engine)" % path)
    lib = C.CDLL(path)
    vp, i32, u64, dp = C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_double)
    lib.cesx_abi_version.restype = C.c_int
    lib.cesx_last_error.restype = C.c_char_p
    lib.cesx_last_error.argtypes = [vp]
    lib.cesx_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.cesx_destroy.argtypes = [vp]
    lib.cesx_destroy.restype = None
    lib.cesx_set_problem.argtypes = [vp, dp, dp, dp, dp, dp]
    lib.cesx_step.argtypes = [vp, C.POINTER(StepParams), vp, vp, vp, vp, i32, vp]
    lib.cesx_result.argtypes = [vp, C.POINTER(StepResult)]
    lib.cesx_moments_len.argtypes = [vp]
    lib.cesx_moments_len.restype = C.c_size_t
    lib.cesx_colsum.argtypes = [vp, vp, vp, vp, vp]
    lib.cesx_set_shift.argtypes = [vp, vp, vp]
    lib.cesx_moments.argtypes = [vp, vp, vp, vp, vp]
    lib.cesx_moments_uu_len.argtypes = [vp]
    lib.cesx_moments_uu_len.restype = C.c_size_t
    lib.cesx_moments_uu.argtypes = [vp, vp, vp, vp, vp]
    lib.cesx_moments_rest.argtypes = [vp, vp, vp, vp, vp]
    lib.cesx_moments_rest_lineal.argtypes = [vp, vp, vp]
    lib.cesx_chol_async.argtypes = [vp, i32, vp, vp]
    lib.cesx_side_stream.argtypes = [vp]
    lib.cesx_side_stream.restype = vp
    lib.cesx_apply.argtypes = [vp, C.POINTER(StepParams), vp, vp, vp, vp, vp, vp]
    lib.cesx_apply_drift.argtypes = [vp, C.POINTER(StepParams), vp, vp, vp, vp, vp, vp]
    lib.cesx_apply_finish.argtypes = [vp, C.POINTER(StepParams), vp, vp, vp, vp, vp]
    lib.cesx_draw_noise.argtypes = [vp, u64, vp, vp]
    lib.cesx_prefetch_noise.argtypes = [vp, u64, vp]
    lib.cesx_moments_uu_chol.argtypes = [vp, C.c_int32, vp, vp, vp, vp]
    lib.cesx_moments_uu_handover.argtypes = [vp, vp, vp, vp, vp]
    lib.cesx_comm_unique_id.argtypes = [vp]
    lib.cesx_comm_init.argtypes = [vp, i32, i32, vp]
    lib.cesx_comm_destroy.argtypes = [vp]
    lib.cesx_comm_nranks.argtypes = [vp]
    lib.cesx_comm_count.argtypes = [vp]
    lib.cesx_comm_stats.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    for name in ("cesx_allreduce_head", "cesx_allreduce_tail", "cesx_allreduce_whole"):
        getattr(lib, name).argtypes = [vp, vp, vp]
    for name in ("cesx_allreduce_sum", "cesx_allreduce_max"):
        getattr(lib, name).argtypes = [vp, vp, C.c_size_t, vp]
    lib.cesx_debug_poll_recoveries.argtypes = [vp]
    lib.cesx_debug_poll_recoveries.restype = C.c_ulonglong
    lib.cesx_debug_warm_inverse.argtypes = [vp]
    lib.cesx_debug_update_form.argtypes = [vp]
    lib.cesx_forward_lineal.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.cesx_forward_set_lineal.argtypes = [vp, vp, vp, vp]
    lib.cesx_forward_apply.argtypes = [vp, vp, vp, vp]
    lib.cesx_debug_dense.argtypes = [vp, dp, dp, dp, dp, dp, dp]
    lib.cesx_debug_gram_plan.argtypes = [i32, i32, i32, i32, i32, C.c_longlong, C.POINTER(C.c_int)]
    lib.cesx_debug_dense_plan.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.cesx_profile_enable.argtypes = [vp, i32]
    lib.cesx_profile_read.argtypes = [vp, i32, dp, C.POINTER(C.c_int)]
    lib.cesx_profile_clock.argtypes = [vp, dp]
    lib.cesx_profile_gap.argtypes = [vp, dp]
    lib.cesx_copy_cols_async.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_size_t, i32, vp]
    lib.cesx_calibrate_mfma.argtypes = [vp, C.c_double, dp, dp, vp]
    lib.cesx_mh_set_proposal.argtypes = [vp, i32, dp, C.c_double]
    lib.cesx_mh_start.argtypes = [vp, vp, vp, vp]
    lib.cesx_mh_propose.argtypes = [vp, u64, vp, vp, vp, vp]
    lib.cesx_mh_accept.argtypes = [vp, u64, vp, vp, vp, vp, vp]
    lib.cesx_mh_stats.argtypes = [vp, C.POINTER(C.c_ulonglong), dp, C.POINTER(C.c_ulonglong)]
    lib.cesx_gp_set.argtypes = [vp, C.POINTER(GpDesc)]
    lib.cesx_gp_predict.argtypes = [vp, vp, vp, vp, i32, vp]
    lib.cesx_gp_start.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.cesx_gp_accept.argtypes = [vp, i32, u64, vp, vp, vp, vp, vp, vp]
    lib.cesx_gp_run.argtypes = [vp, i32, u64, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.cesx_gp_dense_set.argtypes =[vp, C.POINTER(GpDenseDesc)]
    lib.cesx_gp_proj_set.argtypes = [vp, C.POINTER(GpProjDesc)]
    lib.cesx_mh_phi.argtypes = [vp, dp]
    lib.cesx_gp_predict_grad.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp]
    lib.cesx_gp_langevin_start.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    lib.cesx_gp_langevin_propose.argtypes = [vp, u64, vp, vp, vp, vp]
    lib.cesx_gp_langevin_accept.argtypes = [vp, i32, u64, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.cesx_gp_proj_coef.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.cesx_gp_proj_langevin_start.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.cesx_gp_proj_langevin_accept.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.cesx_gp_proj_hmc_leap.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.cesx_gp_proj_hmc_accept.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.cesx_gpfit_set.argtypes = [vp, C.POINTER(GpFitDesc)]
    lib.cesx_gpfit_ntheta.argtypes = [vp]
    lib.cesx_gpfit_eval.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    lib.cesx_gpfit_factors.argtypes = [vp, i32, vp, vp]
    lib.cesx_darcy_set.argtypes = [vp, C.POINTER(DarcyDesc)]
    lib.cesx_darcy_apply.argtypes = [vp, vp, vp, vp, vp]
    lib.cesx_darcy_set_streamed.argtypes = [vp, C.POINTER(DarcyDesc), C.c_int]
    lib.cesx_darcy_grad.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.cesx_darcy_grad_lds_bytes.argtypes = [C.c_int]
    lib.cesx_darcy_grad_lds_bytes.restype = C.c_size_t
    lib.cesx_darcy_workspace_bytes.argtypes = [vp]
    lib.cesx_darcy_workspace_bytes.restype = C.c_size_t
    lib.cesx_lorenz_set.argtypes = [vp, C.POINTER(L96Desc)]
    lib.cesx_lorenz_apply.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.cesx_lorenz_three_set.argtypes = [vp, C.POINTER(L63Desc)]
    lib.cesx_lorenz_three_apply.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.cesx_map_set.argtypes = [vp, C.POINTER(MapDesc)]
    lib.cesx_map_apply.argtypes = [vp, vp, vp, vp]
    lib.cesx_mh_run_map.argtypes = [vp, u64, i32, i32, vp, vp, vp, vp, vp]
    lib.cesx_map_jac.argtypes = [vp, vp, vp, vp, vp]
    lib.cesx_mh_langevin_start.argtypes = [vp, vp, vp, vp, vp]
    lib.cesx_mh_langevin_propose.argtypes = [vp, u64, vp, vp, vp, vp]
    lib.cesx_mh_langevin_accept.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]
    lib.cesx_mh_langevin_run_map.argtypes = [vp, u64, i32, i32, vp, vp, vp, vp, vp]
    lib.cesx_mh_langevin_lineal_set.argtypes = [vp, dp, dp, i32]
    lib.cesx_mh_langevin_lineal_start.argtypes = [vp, vp, vp, vp]
    lib.cesx_mh_langevin_lineal_propose.argtypes = [vp, u64, vp, vp, vp, vp]
    lib.cesx_mh_langevin_lineal_accept.argtypes = [vp, u64, vp, vp, vp, vp, vp]
    lib.cesx_mh_langevin_lineal_g.argtypes = [vp, dp]
    lib.cesx_mh_hmc_lineal_begin.argtypes = [vp, u64, vp, vp, vp, vp]
    lib.cesx_mh_hmc_lineal_leap.argtypes = [vp, vp, vp, vp, vp]
    lib.cesx_mh_hmc_lineal_accept.argtypes = [vp, u64, vp, vp, vp, vp, vp]
    lib.cesx_mh_hmc_begin.argtypes = [vp, u64, vp, vp, vp, vp]
    lib.cesx_mh_hmc_leap.argtypes = [vp, vp, vp, vp, vp]
    lib.cesx_mh_hmc_accept.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]
    lib.cesx_gp_hmc_leap.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    lib.cesx_gp_hmc_accept.argtypes = [vp, i32, u64, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.cesx_mh_hmc_run_map.argtypes = [vp, u64, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.cesx_mh_adapt_set.argtypes = [vp, i32, C.c_double, C.c_double, C.c_double]
    lib.cesx_mh_adapt_read.argtypes = [vp, dp, C.POINTER(C.c_int32), dp]
    lib.cesx_mh_grad_source.argtypes = [vp, i32]
    lib.cesx_chain_summary_begin.argtypes = [vp, i32, vp]
    lib.cesx_chain_summary_add.argtypes = [vp, vp, i32, vp]
    lib.cesx_chain_summary_read.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.cesx_chain_hist_begin.argtypes = [vp, vp, vp]
    lib.cesx_chain_hist_add.argtypes = [vp, vp, i32, vp]
    lib.cesx_chain_hist_read.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.cesx_chain_acf_begin.argtypes = [vp, i32, i32, i32, vp]
    lib.cesx_chain_acf_add.argtypes = [vp, vp, i32, vp]
    lib.cesx_chain_acf_read.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    if lib.cesx_abi_version() != ABI_VERSION:
        raise ImportError("libcesx.so ABI %d != binding ABI %d" % (lib.cesx_abi_version(), ABI_VERSION))
    if path == LIB_PATH:
        _lib = lib
    return lib


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def step_params(update="aldi", time_step=None, first_step=True, t_len=0, t_last=0.0, delta_t=None,
                spinup=4.0, switch=1.0, step_index=0, T=30):
    """kwargs of sampling.eks_update* (ces/calibrate.py:247-260, :517) -> cesx_step_params."""
    if update not in UPDATES:
        raise ValueError("unknown update rule %r" % (update,))
    if time_step not in TIME_STEPS:
        # the reference leaves hk unbound for unknown strings (ces/calibrate.py:262)
        raise UnboundLocalError("local variable 'hk' referenced before assignment")
    prm = StepParams()
    prm.struct_bytes = C.sizeof(StepParams)
    prm.update = UPDATES[update]
    prm.time_step = TIME_STEPS[time_step]
    prm.first_step = int(bool(first_step))
    prm.t_len = int(t_len)
    prm.t_last = float(t_last)
    prm.delta_t = float(delta_t if delta_t is not None else 1.0 / (T / 2))
    prm.spinup = float(spinup)
    prm.switch_mult = float(switch)
    prm.step_index = int(step_index)
    return prm


class Engine:
    """One handle = one device = one particle shard (cesx_create)."""

    def __init__(self, p, n_obs, J, dtype="float32", device=0, J_global=None, j_offset=0, seed=1234):
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("ces_amd needs a HIP device: the ensemble update has no CPU path")
        self.p, self.n_obs, self.J = int(p), int(n_obs), int(J)
        self.J_global = int(J_global if J_global is not None else J)
        self.np_dtype = np.dtype(dtype)
        if self.np_dtype not in (np.dtype("float32"), np.dtype("float64")):
            raise ValueError("dtype must be float32 or float64")
        self.torch_dtype = torch.float32 if self.np_dtype == np.dtype("float32") else torch.float64
        self.device = torch.device("cuda", int(device))
        self._dev_index = int(device)
        cfg = Config()
        cfg.struct_bytes = C.sizeof(Config)
        cfg.p, cfg.n_obs = self.p, self.n_obs
        cfg.dtype = F32 if self.np_dtype == np.dtype("float32") else F64
        cfg.device = int(device)
        cfg.J_local, cfg.J_global, cfg.j_offset = self.J, self.J_global, int(j_offset)
        cfg.seed = int(seed)
        self._h = C.c_void_p()
        rc = self.lib.cesx_create(C.byref(cfg), C.byref(self._h))
        if rc != OK:
            raise CesxError(rc, self.lib.cesx_last_error(None).decode())
        self._problem = None
        self._chain_hist_shape = None      # (bins, bins2d, pairs) of the run of histograms in hand
        self._keep_chain_hist = None
        self._chain_acf_shape = None       # (lags, chains) of the run of lagged sums in hand
        self._keep_chain_acf = None

    def close(self):
        """Destroy the handle and free its device memory now (what garbage collection would do later)."""
        self.__del__()

    def __del__(self):
        pool = self.__dict__.pop("_out_pool", None)
        if pool is not None:
            pool.close()
        h, self._h = getattr(self, "_h", None), None
        if h:
            self.lib.cesx_destroy(h)

    # -- helpers ---------------------------------------------------------
    def _check(self, rc):
        if rc == OK:
            return
        msg = self.lib.cesx_last_error(self._h).decode()
        if rc == ENOTPD:
            raise np.linalg.LinAlgError(msg or "Matrix is not positive definite")
        if rc == ENOCONV:                 # what np.linalg.eigvals (ces/calibrate.py:250) raises
            raise np.linalg.LinAlgError("Eigenvalues did not converge: " + msg)
        if rc == EUNSUPPORTED:
            raise AttributeError("'sampling' object has no attribute 'LM_procedure'")
        if rc == EINVAL:
            raise ValueError(msg)
        raise CesxError(rc, msg)

    def _stream(self):
        # (the raw handle of torch's current stream: ~0.3 us through the C binding, 2 us through the Stream object --
        #  a step of a small problem is bound by the driving thread, tools/host_call_cost.py)
        raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        if raw is not None:
            return C.c_void_p(raw(self._dev_index))
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # Host arrays cross PCIe through persistent pinned staging buffers in the ENGINE dtype: the
    # cast float64 -> engine dtype is a multi-threaded torch copy into the pinned buffer (1.4 ms
    # for a 256 x 65 536 block, against 11 ms for numpy astype + a pageable upload), the way back
    # is pinned engine-dtype -> float64 on the host (3.9 ms against 32 ms).  Large blocks only.
    _PIN_MIN = 1 << 16         # from here on: multi-threaded torch casts, chunked D2H into pre-faulted result arrays
    _PIN_SMALL = 1 << 10       # ... and from here on pinned staging at all (numpy's own cast; the reference's sizes, J <= 768)
    copy_threads = default_copy_threads()     # host threads for the staging casts (see default_copy_threads)

    class _HostThreads:
        """Bound torch's intra-op thread count for a host-side copy (a 128-thread pool on a
        16-core CPU share turned 2 ms casts into 90 ms ones)."""

        def __init__(self, n):
            self.n = n

        def __enter__(self):
            self.old = torch.get_num_threads()
            if self.old > self.n:
                torch.set_num_threads(self.n)

        def __exit__(self, *exc):
            if torch.get_num_threads() != self.old:
                torch.set_num_threads(self.old)

    def _pinned(self, tag, shape):
        pool = self.__dict__.setdefault("_pin_pool", {})
        key = (tag, tuple(shape))
        if key not in pool:
            try:
                pool[key] = torch.empty(shape, dtype=self.torch_dtype).pin_memory()
            except RuntimeError:
                pool[key] = None                         # no pinned memory left: pageable path
        return pool[key]

    def to_device(self, a, rows=None, tag="in"):
        """Host (rows, J) array or device tensor -> contiguous device tensor of the engine dtype."""
        if isinstance(a, torch.Tensor):
            t = a.to(device=self.device, dtype=self.torch_dtype).contiguous()
        else:
            a = np.asarray(a)
            pin = self._pinned(tag, a.shape) if a.size >= self._PIN_SMALL and a.dtype.kind == "f" else None
            if pin is not None and a.size < self._PIN_MIN:
                # small arrays: cast straight into the pinned buffer with numpy (no torch thread-pool juggling, no pageable
                # staging copy inside the runtime: ~10 us instead of ~25 per array), asynchronous H2D out of it
                evs = self.__dict__.setdefault("_pin_events", {})
                key = (tag, tuple(a.shape))
                if key in evs:
                    evs[key].synchronize()
                views = self.__dict__.setdefault("_pin_views", {})
                view = views.get(key)
                if view is None:
                    view = views[key] = pin.numpy()
                np.copyto(view, a, casting="unsafe")
                with torch.cuda.device(self.device):
                    t = pin.to(self.device, non_blocking=True)
                    ev = evs.get(key)
                    if ev is None:
                        ev = evs[key] = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream(self.device))
            elif pin is not None:
                # Asynchronous H2D out of the tag's own staging buffer: the cast of the NEXT array (another tag)
                # runs on the host while this one crosses PCIe.  The buffer is written again only after the event
                # of its last copy has completed.
                evs = self.__dict__.setdefault("_pin_events", {})
                key = (tag, tuple(a.shape))
                if key in evs:
                    evs[key].synchronize()
                with self._HostThreads(self.copy_threads):
                    pin.copy_(torch.from_numpy(np.ascontiguousarray(a)))
                with torch.cuda.device(self.device):
                    t = pin.to(self.device, non_blocking=True)
                    ev = evs.get(key)
                    if ev is None:
                        ev = evs[key] = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream(self.device))
            else:
                t = torch.as_tensor(np.ascontiguousarray(a, dtype=self.np_dtype), device=self.device)
        if rows is not None and tuple(t.shape) != (rows, self.J):
            raise ValueError("expected shape (%d, %d), got %s" % (rows, self.J, tuple(t.shape)))
        return t

    class _HostOutPool:
        """Fresh float64 result arrays, page-faulted AHEAD of use by a helper thread.

        The reference returns a newly allocated (p, J) float64 array from every update
        (ces/calibrate.py:443/:484/:525 build ``Uk`` from temporaries) and the trace keeps it alive, so
        the drop-in must hand out fresh memory too -- and at J = 65 536, p = 256 the first touch of 134 MB
        of new pages costs 12-20 ms, more than everything else in the call together.  The pool keeps a
        few arrays per shape allocated and touched by a background thread; ``get`` is then a list pop.
        One ready list per shape (a trace of U (p, J) and G (n, J) alternates two shapes); the two most recently
        asked-for shapes are kept, older ones are dropped on the helper thread.  All counters are guarded by one
        condition variable; ``get`` never waits longer than ``wait_s`` for the helper (it allocates itself then)."""

        keep_shapes = 2
        wait_s = 2.0

        def __init__(self, depth=2):
            import queue
            import threading
            self.depth = depth
            self.shape = None                     # the shape asked for last
            self.recycled = 0
            self.cv = threading.Condition()
            self.ready = {}                       # shape -> arrays with their pages mapped (insertion order = LRU)
            self.pending = {}                     # shape -> fresh arrays asked for and not yet delivered
            self.req = queue.Queue()
            self.th = threading.Thread(target=self._work, daemon=True, name="cesx-hostpool")
            self.th.start()

        def close(self):
            """Stop the helper thread and release the prepared arrays (Engine.__del__)."""
            self.req.put(None)
            with self.cv:
                self.ready.clear()
                self.pending.clear()

        _touch_pool = None

        @classmethod
        def _fresh(cls, shape, threads=8):
            a = np.empty(shape, dtype=np.float64)
            flat = a.reshape(-1)
            n = flat.size
            if n < (1 << 22):
                flat[::512] = 0.0                   # one write per 4 KiB page: the kernel maps (and zeroes) it now
                return a
            # the kernel zeroes every new page (~10 GB/s per faulting thread): touch slices from several threads
            if cls._touch_pool is None:
                from concurrent.futures import ThreadPoolExecutor
                cls._touch_pool = ThreadPoolExecutor(max_workers=threads, thread_name_prefix="cesx-prefault")
            step = (n // threads + 511) // 512 * 512

            def touch(k):
                flat[k * step:min(n, (k + 1) * step):512] = 0.0
            list(cls._touch_pool.map(touch, range((n + step - 1) // step)))
            return a

        def _work(self):
            while True:
                item = self.req.get()
                if item is None:
                    return
                if isinstance(item, list):           # arrays handed over by discard()
                    self._take_back(item)
                    continue
                with self.cv:
                    wanted = item in self.ready       # (the shape may have been evicted since it was asked for)
                a = self._fresh(item) if wanted else None
                with self.cv:
                    self.pending[item] = max(0, self.pending.get(item, 0) - 1)
                    if a is not None and item in self.ready:
                        self.ready[item].append(a)
                    self.cv.notify_all()
                del a

        def _take_back(self, arrays):
            """Arrays the caller is done with.  One that nobody else refers to, of a shape being handed out, goes
            back into that shape's ready list -- its pages are mapped, the next ``get`` costs neither a page fault
            nor, here, an ``munmap`` (together 16-20 ms per 134 MB array and iteration); anything else is dropped
            (unmapped) on this thread.  The caller drops its own references right after ``discard`` returns: wait
            for that."""
            import sys
            import time
            while arrays:
                a = arrays.pop()
                ok = isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.owndata and a.flags.c_contiguous
                if ok:
                    with self.cv:
                        lst = self.ready.get(tuple(a.shape))
                        ok = lst is not None and len(lst) <= self.depth
                if ok:
                    for _ in range(20):                      # holders: `a` and getrefcount's argument
                        if sys.getrefcount(a) <= 2:
                            break
                        time.sleep(0.0005)
                    ok = sys.getrefcount(a) <= 2
                if ok:
                    with self.cv:
                        lst = self.ready.get(tuple(a.shape))
                        if lst is not None:
                            lst.append(a)
                            self.recycled += 1
                            self.cv.notify_all()
                del a

        def discard(self, arrays):
            """Drop large host arrays on the helper thread: unmapping 134 MB takes ~8 ms on the caller's
            thread otherwise (the caller must not keep a reference of its own)."""
            if self.th.is_alive():
                self.req.put(list(arrays))

        def _top_up(self, shape):
            """(lock held) ask the helper for fresh arrays until ready + pending reaches the depth."""
            want = self.depth - len(self.ready[shape]) - self.pending.get(shape, 0)
            for _ in range(max(0, want)):
                self.pending[shape] = self.pending.get(shape, 0) + 1
                self.req.put(shape)

        def get(self, shape):
            import time
            shape = tuple(int(x) for x in shape)
            if not self.th.is_alive():
                return self._fresh(shape)
            dropped = []
            with self.cv:
                self.shape = shape
                lst = self.ready.pop(shape, None)
                self.ready[shape] = lst if lst is not None else []        # (re-inserted: most recently used)
                while len(self.ready) > self.keep_shapes:                  # evict the least recently used shape
                    old = next(iter(self.ready))
                    dropped.extend(self.ready.pop(old))
                    self.pending.pop(old, None)
                self._top_up(shape)
                deadline = time.monotonic() + self.wait_s
                while not self.ready[shape]:
                    left = deadline - time.monotonic()
                    if left <= 0 or not self.th.is_alive():
                        break
                    self.cv.wait(min(left, 0.05))
                a = self.ready[shape].pop() if self.ready[shape] else None
                self._top_up(shape)
            if dropped:
                self.req.put(dropped)                                      # unmapped on the helper thread
            return a if a is not None else self._fresh(shape)

    def _host_pool(self):
        """The engine's one result-array pool (created on first use; its helper thread ends with the engine)."""
        pool = self.__dict__.get("_out_pool")
        if pool is None:
            pool = self._out_pool = self._HostOutPool()
        return pool

    def to_host(self, t):
        """Device tensor of the engine dtype -> NEW float64 numpy array (the reference's dtype)."""
        pin = self._pinned("out", t.shape) if t.numel() >= self._PIN_SMALL else None
        if pin is None:
            return t.to("cpu", dtype=torch.float64).numpy()
        if t.numel() < self._PIN_MIN:
            # small: one asynchronous D2H into pinned memory, then numpy's own widening into a fresh array
            evs = self.__dict__.setdefault("_out_events", [])
            with torch.cuda.device(self.device):
                pin.copy_(t, non_blocking=True)
                if not evs:
                    evs.append(torch.cuda.Event())
                evs[0].record(torch.cuda.current_stream(self.device))
            evs[0].synchronize()
            return pin.numpy().astype(np.float64)
        # D2H into pinned memory in row chunks, each widened into the result array (pages already mapped) while the
        # next one is still crossing PCIe
        rows = int(t.shape[0])
        nchunk = 4 if rows >= 8 else 1
        step = (rows + nchunk - 1) // nchunk
        evs = self.__dict__.setdefault("_out_events", [])
        parts = []
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device)
            for k in range(nchunk):
                sl = slice(k * step, min(rows, (k + 1) * step))
                if sl.start >= sl.stop:
                    break
                pin[sl].copy_(t[sl], non_blocking=True)
                if len(evs) <= k:
                    evs.append(torch.cuda.Event())
                evs[k].record(st)
                parts.append((sl, evs[k]))
        out = self._host_pool().get(tuple(t.shape))
        dst = torch.from_numpy(out)
        with self._HostThreads(self.copy_threads):
            for sl, ev in parts:
                ev.synchronize()
                dst[sl].copy_(pin[sl])
        return out

    def discard_host(self, *arrays):
        """Hand large host arrays the caller no longer needs to the helper thread for release."""
        self._host_pool().discard([a for a in arrays if isinstance(a, np.ndarray) and a.nbytes >= (1 << 22)])

    def copy_cols_async(self, dst, src, a, b, to_device, stream=None):
        """Columns [a, b) of a row-major 2-D tensor between a PINNED host tensor and a device tensor of the same shape,
        asynchronously on ``stream`` (cesx_copy_cols_async; torch's own non_blocking copy of a strided block blocks the
        host for the whole transfer)."""
        esz = dst.element_size()
        rows = int(dst.shape[0])
        st = self._stream() if stream is None else C.c_void_p(stream)
        self._check(self.lib.cesx_copy_cols_async(self._h, dst.data_ptr() + a * esz, int(dst.stride(0)) * esz,
                                               src.data_ptr() + a * esz, int(src.stride(0)) * esz,
                                               (b - a) * esz, rows, int(bool(to_device)), st))

    def empty(self, rows):
        return torch.empty((rows, self.J), dtype=self.torch_dtype, device=self.device)

    # -- problem ---------------------------------------------------------
    def set_problem(self, y, Gamma, mu, sigma, ustar):
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(self.n_obs))
        Gamma = np.ascontiguousarray(np.asarray(Gamma, dtype=np.float64).reshape(self.n_obs, self.n_obs))
        mu = np.ascontiguousarray(np.asarray(mu, dtype=np.float64).reshape(self.p))
        sigma = np.asarray(sigma, dtype=np.float64)
        if sigma.ndim == 0:
            sigma = float(sigma) * np.eye(self.p)
        sigma = np.ascontiguousarray(sigma.reshape(self.p, self.p))
        ustar = np.ascontiguousarray(np.asarray(ustar, dtype=np.float64).reshape(self.p))
        key = (y, Gamma, mu, sigma, ustar)
        if self._problem is not None and all(np.array_equal(a, b) for a, b in zip(key, self._problem)):
            return
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_set_problem(self._h, _dptr(y), _dptr(Gamma), _dptr(mu), _dptr(sigma),
                                                  _dptr(ustar)))
        self._problem = tuple(a.copy() for a in key)
        # a dense Gamma: the engine whitens the data once per step and runs the diagonal path (include/cesx.h)
        self.dense_gamma = bool(np.count_nonzero(Gamma - np.diag(np.diagonal(Gamma))))

    # -- single device step ------------------------------------------------
    def step(self, prm, U, G, xi=None, out=None, recenter=True):
        """cesx_step: returns the new (p, J) device tensor (never aliases U)."""
        U, G = self.to_device(U, self.p, "U"), self.to_device(G, self.n_obs, "G")
        xi_t = None if xi is None else self.to_device(xi, self.p, "xi")
        out = self.empty(self.p) if out is None else out
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_step(self._h, C.byref(prm), U.data_ptr(), G.data_ptr(),
                                           None if xi_t is None else xi_t.data_ptr(), out.data_ptr(),
                                           int(bool(recenter)), self._stream()))
        self._keep = (U, G, xi_t, out)      # keep inputs alive until the stream has consumed them
        return out

    def result(self):
        res = StepResult()
        rc = self.lib.cesx_result(self._h, C.byref(res))
        if rc == ESTATE and self.poll_recoveries() > self.__dict__.get("_seen_recoveries", 0):
            # a polled join ran out, the step was re-run and `res` is valid; moments enqueued behind it must be redone
            # (include/cesx.h): the pipelined drivers (ShardedUpdate.result) do that and carry on
            self._seen_recoveries = self.poll_recoveries()
            raise CesxError(rc, self.lib.cesx_last_error(self._h).decode(), result=res)
        self._seen_recoveries = self.poll_recoveries()
        self._check(rc)
        return res

    # -- split entry points -------------------------------------------------
    def moments_len(self):
        return int(self.lib.cesx_moments_len(self._h))

    def colsum(self, U, G):
        sums = torch.empty(1 + self.p + self.n_obs, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_colsum(self._h, U.data_ptr(), G.data_ptr(), sums.data_ptr(), self._stream()))
        return sums

    def set_shift(self, sums):
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_set_shift(self._h, sums.data_ptr(), self._stream()))

    def moments(self, U, G, out=None):
        mom = torch.empty(self.moments_len(), dtype=torch.float64, device=self.device) if out is None else out
        self._check(self.lib.cesx_moments(self._h, U.data_ptr(), G.data_ptr(), mom.data_ptr(), self._stream()))
        return mom

    def moments_uu_len(self):
        return int(self.lib.cesx_moments_uu_len(self._h))

    def side_stream(self):
        """The engine's side stream as a torch stream (cesx_side_stream)."""
        return torch.cuda.ExternalStream(int(self.lib.cesx_side_stream(self._h)), device=self.device)

    def moments_uu(self, U, G, out=None):
        """U x U part of the moments into the leading moments_uu_len() entries of the buffer."""
        mom = torch.empty(self.moments_len(), dtype=torch.float64, device=self.device) if out is None else out
        self._check(self.lib.cesx_moments_uu(self._h, U.data_ptr(), G.data_ptr(), mom.data_ptr(), self._stream()))
        return mom

    def chol_async(self, prm, mom):
        """C = cov(U) and L = chol(C) on the engine's side stream (joined by apply)."""
        self._check(self.lib.cesx_chol_async(self._h, int(prm.update), mom.data_ptr(), self._stream()))

    def moments_uu_chol(self, prm, U, G, out=None):
        """moments_uu + chol_async in one call (one device, nothing between the two: cesx_moments_uu_chol)."""
        mom = torch.empty(self.moments_len(), dtype=torch.float64, device=self.device) if out is None else out
        self._check(self.lib.cesx_moments_uu_chol(self._h, int(prm.update), U.data_ptr(), G.data_ptr(),
                                                  mom.data_ptr(), self._stream()))
        return mom

    # -- the exchange step of a sharded ensemble behind the C ABI (RCCL; include/cesx.h cesx_comm_*) --
    COMM_ID_BYTES = 128

    def comm_unique_id(self):
        """Rank 0: the 128-byte id every rank passes to ``comm_init`` (ncclGetUniqueId)."""
        buf = C.create_string_buffer(self.COMM_ID_BYTES)
        rc = self.lib.cesx_comm_unique_id(buf)
        if rc != OK:
            raise CesxError(rc, "cesx_comm_unique_id failed (librccl.so not loadable?)")
        return bytes(buf.raw)

    def comm_init(self, nranks, rank, unique_id):
        """Collective over the ranks: an RCCL communicator on this engine's device (ncclCommInitRank)."""
        assert len(unique_id) == self.COMM_ID_BYTES
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_comm_init(self._h, int(nranks), int(rank), C.c_char_p(unique_id)))

    def comm_destroy(self):
        self._check(self.lib.cesx_comm_destroy(self._h))

    def comm_nranks(self):
        return int(self.lib.cesx_comm_nranks(self._h))

    def comm_count(self):
        """Communicators the engine holds: 2 = one per stream (main + side), 1 = shared, 0 = none (cesx_comm_count)."""
        return int(self.lib.cesx_comm_count(self._h))

    def comm_stats(self):
        """(all-reduces issued through the engine's communicator so far, their total payload in doubles)."""
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        self._check(self.lib.cesx_comm_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def allreduce(self, t, op="sum", part=None):
        """In-place RCCL all-reduce on the current stream through the engine's communicator.  ``part`` in
        {"head", "tail", "whole"}: ``t`` is the whole moment buffer and the named piece of it is summed
        (cesx_allreduce_head / _tail / _whole); otherwise ``t`` is any contiguous float64 device tensor."""
        assert t.dtype == torch.float64 and t.is_contiguous()
        if part is not None:
            fn = {"head": self.lib.cesx_allreduce_head, "tail": self.lib.cesx_allreduce_tail, "whole": self.lib.cesx_allreduce_whole}[part]
            assert t.numel() == self.moments_len()
            self._check(fn(self._h, t.data_ptr(), self._stream()))
        else:
            fn = self.lib.cesx_allreduce_max if op == "max" else self.lib.cesx_allreduce_sum
            self._check(fn(self._h, t.data_ptr(), t.numel(), self._stream()))
        return t

    def warm_inverse(self):
        """1 when the last hk-dependent SPD inverse of a step came from the warm start (cesx_debug_warm_inverse)."""
        return int(self.lib.cesx_debug_warm_inverse(self._h))

    def update_form(self):
        """Form of the update GEMM the last step launched: 0 assembled, 1 hk-free, 2 through the Cholesky factor
        (cesx_debug_update_form)."""
        return int(self.lib.cesx_debug_update_form(self._h))

    def poll_recoveries(self):
        """Steps whose polled join of the side stream ran out and that cesx_result re-ran (include/cesx.h)."""
        return int(self.lib.cesx_debug_poll_recoveries(self._h))

    def moments_uu_handover(self, U, G, out=None):
        """moments_uu on the current stream, then the engine's side stream waits for it (cesx_moments_uu_handover)."""
        mom = torch.empty(self.moments_len(), dtype=torch.float64, device=self.device) if out is None else out
        self._check(self.lib.cesx_moments_uu_handover(self._h, U.data_ptr(), G.data_ptr(), mom.data_ptr(), self._stream()))
        return mom

    def moments_rest(self, U, G, mom):
        self._check(self.lib.cesx_moments_rest(self._h, U.data_ptr(), G.data_ptr(), mom.data_ptr(), self._stream()))
        return mom

    def moments_rest_lineal(self, mom):
        """The G part of the moments from the head of ``mom`` and the installed linear map (cesx_moments_rest_lineal)."""
        self._check(self.lib.cesx_moments_rest_lineal(self._h, mom.data_ptr(), self._stream()))
        return mom

    def apply(self, prm, mom, U, G, xi=None, out=None):
        out = self.empty(self.p) if out is None else out
        self._check(self.lib.cesx_apply(self._h, C.byref(prm), mom.data_ptr(), U.data_ptr(), G.data_ptr(),
                                        None if xi is None else xi.data_ptr(), out.data_ptr(), self._stream()))
        self._keep = (mom, U, G, xi, out)
        return out

    def apply_drift(self, prm, mom, U, G, out):
        absmax = torch.empty(1, dtype=torch.float64, device=self.device)
        self._check(self.lib.cesx_apply_drift(self._h, C.byref(prm), mom.data_ptr(), U.data_ptr(),
                                              G.data_ptr(), out.data_ptr(), absmax.data_ptr(), self._stream()))
        return absmax

    def apply_finish(self, prm, absmax, U, xi, out):
        self._check(self.lib.cesx_apply_finish(self._h, C.byref(prm), absmax.data_ptr(), U.data_ptr(),
                                               None if xi is None else xi.data_ptr(), out.data_ptr(),
                                               self._stream()))
        self._keep = (absmax, U, xi, out)
        return out

    def draw_noise(self, step_index):
        xi = self.empty(self.p)
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_draw_noise(self._h, int(step_index), xi.data_ptr(), self._stream()))
        return xi

    def prefetch_noise(self, step_index):
        """Draw the noise block of ``step_index`` ahead of its update (cesx_prefetch_noise)."""
        self._check(self.lib.cesx_prefetch_noise(self._h, int(step_index), self._stream()))

    def forward_lineal(self, A, U, b=None, out=None):
        A = torch.as_tensor(A).to(device=self.device, dtype=self.torch_dtype).contiguous()
        if tuple(A.shape) != (self.n_obs, self.p):
            raise ValueError("A must be (n_obs, p)")
        bt = None if b is None else torch.as_tensor(b).to(device=self.device, dtype=self.torch_dtype).reshape(-1).contiguous()
        out = self.empty(self.n_obs) if out is None else out
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_forward_lineal(self._h, A.data_ptr(), None if bt is None else bt.data_ptr(),
                                                     U.data_ptr(), out.data_ptr(), self._stream()))
        self._keep = (A, bt, U, out)
        return out

    def forward_set_lineal(self, A, b=None):
        """Install the linear map G = A U + b in the engine (cesx_forward_set_lineal); the engine keeps its own copy."""
        A = torch.as_tensor(A).to(device=self.device, dtype=self.torch_dtype).contiguous()
        if tuple(A.shape) != (self.n_obs, self.p):
            raise ValueError("A must be (n_obs, p)")
        bt = None if b is None else torch.as_tensor(np.ascontiguousarray(b)).to(device=self.device, dtype=self.torch_dtype).reshape(-1).contiguous()
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_forward_set_lineal(self._h, A.data_ptr(), None if bt is None else bt.data_ptr(),
                                                         self._stream()))
            torch.cuda.current_stream(self.device).synchronize()       # A, bt may be released now
        self._fwd_token = object()          # identifies the installed map (ces_amd.utils.lineal checks it)
        return self._fwd_token

    def forward_apply(self, U, out=None):
        """G = A U + b with the installed map (cesx_forward_apply)."""
        out = self.empty(self.n_obs) if out is None else out
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_forward_apply(self._h, U.data_ptr(), out.data_ptr(), self._stream()))
        self._keep_fwd = (U, out)
        return out

    # -- Metropolis-Hastings over the columns (include/cesx.h, cesx_mh_*; ces_amd/sample.py drives it) --
    def mh_set_proposal(self, update, S, beta=0.5):
        """The proposal of MCMC.model_mh: update None (random walk, P = U + S xi) or 'pCN' (P = sqrt(1 - beta^2) U +
        sqrt(beta) S xi); S the p x p lower-triangular scales (cesx_mh_set_proposal)."""
        if update not in MH_KINDS:
            raise ValueError("unknown MH update %r" % (update,))
        S = np.ascontiguousarray(np.asarray(S, dtype=np.float64).reshape(self.p, self.p))
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_set_proposal(self._h, MH_KINDS[update], _dptr(S), float(beta)))

    def mh_start(self, U, G):
        """phi of the current states U with their forward map G; the accept counters cleared (cesx_mh_start)."""
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_start(self._h, U.data_ptr(), G.data_ptr(), self._stream()))
        self._keep_mh = (U, G)

    def mh_propose(self, step_index, U, xi=None, out=None):
        """P = a U + b S xi (cesx_mh_propose); xi None: drawn on device in the MH counter domain of step_index."""
        out = self.empty(self.p) if out is None else out
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_propose(self._h, int(step_index), U.data_ptr(),
                                                 None if xi is None else xi.data_ptr(), out.data_ptr(), self._stream()))
        self._keep_mh_p = (U, xi, out)
        return out

    def mh_accept(self, step_index, U, P, GP, logu=None):
        """phi(P), the test log u < phi(U) - phi(P), U := P on the accepted columns (cesx_mh_accept); logu None: the
        device uniform of step_index, else a float64 device tensor of J values."""
        if logu is not None:
            assert logu.dtype == torch.float64 and logu.numel() == self.J and logu.is_contiguous()
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_accept(self._h, int(step_index), U.data_ptr(), P.data_ptr(), GP.data_ptr(),
                                                None if logu is None else logu.data_ptr(), self._stream()))
        self._keep_mh_a = (U, P, GP, logu)

    def mh_stats(self, per_chain=False):
        """(accept calls since mh_start, overall accept rate[, per-chain counters]) (cesx_mh_stats; synchronises)."""
        steps, rate = C.c_ulonglong(0), C.c_double(0.0)
        buf = np.zeros(self.J, dtype=np.uint64) if per_chain else None
        self._check(self.lib.cesx_mh_stats(self._h, C.byref(steps), C.byref(rate),
                                           None if buf is None else buf.ctypes.data_as(C.POINTER(C.c_ulonglong))))
        if per_chain:
            return int(steps.value), rate.value, buf
        return int(steps.value), rate.value

    def mh_phi(self):
        """The J current phi values of the chains, float64 on the host (cesx_mh_phi; synchronises)."""
        buf = np.zeros(self.J, dtype=np.float64)
        self._check(self.lib.cesx_mh_phi(self._h, _dptr(buf)))
        return buf

    # -- GP emulator over the columns (include/cesx.h, cesx_gp_*; ces_amd/emulate.py and ces_amd/sample.py drive it) --
    def gp_set(self, img):
        """Install an emulator: ``img`` as ``ces_amd.emulate.device_image`` returns it (cesx_gp_set)."""
        n, Jt, p = int(img["n"]), int(img["Jt"]), self.p
        if int(img["p"]) != p:
            raise ValueError("gp_set: the emulator's input dimension %d differs from p = %d" % (img["p"], p))
        arr = {k: np.ascontiguousarray(np.asarray(img[k], dtype=np.float64))
               for k in ("A", "c", "Z", "par", "mw", "alpha", "Li")}
        fam = np.ascontiguousarray(np.asarray(img["family"], dtype=np.int32).reshape(n))
        shapes = dict(A=(n, p, p), c=(p,), Z=(n, Jt, p), par=(n, 3), mw=(n, p), alpha=(n, Jt), Li=(n, Jt, Jt))
        for k, s in shapes.items():
            if arr[k].shape != s:
                raise ValueError("gp_set: %s has shape %s, expected %s" % (k, arr[k].shape, s))
        d = GpDesc(C.sizeof(GpDesc), n, Jt, *[arr[k].ctypes.data for k in ("A", "c", "Z")], fam.ctypes.data,
                   *[arr[k].ctypes.data for k in ("par", "mw", "alpha", "Li")])
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_gp_set(self._h, C.byref(d)))
        self.gp_n = n

    def gp_dense_set(self, B, g0=None, logdet=False):
        """The descriptor of mode 'dense' (cesx_gp_dense_set): B (n_obs, k), the data space's basis (pca_tools['VD_k']); g0
        (n_obs,) its shift (pca_tools['mG']) or None; logdet: add 1/2 log det Sigma.  Needs the problem; a later set_problem
        drops it.  In mode 'dense' gp_start / gp_accept take (k, J) mean and variance rows."""
        B = np.ascontiguousarray(np.asarray(B, dtype=np.float64))
        if B.ndim != 2 or B.shape[0] != self.n_obs:
            raise ValueError("gp_dense_set: B has shape %s, expected (%d, k)" % (B.shape, self.n_obs))
        if g0 is not None:
            g0 = np.ascontiguousarray(np.asarray(g0, dtype=np.float64).reshape(-1))
            if g0.shape != (self.n_obs,):
                raise ValueError("gp_dense_set: g0 has %d values, expected %d" % (g0.size, self.n_obs))
        d = GpDenseDesc(C.sizeof(GpDenseDesc), B.shape[1], 1 if logdet else 0, B.ctypes.data if B.size else None,
                        None if g0 is None else g0.ctypes.data)
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_gp_dense_set(self._h, C.byref(d)))

    def gp_proj_set(self, R, a0, c_perp, half_logdet_gamma, logdet=False):
        """The descriptor of mode 'proj' (cesx_gp_proj_set), as ``ces_amd.emulate.project_sigma`` returns it: R (k, k) upper
        triangular, a0 (k,), c_perp >= 0 and half_logdet_gamma; logdet: add 1/2 log det Sigma.  Needs the problem; a later
        set_problem drops it.  In mode 'proj' gp_start / gp_accept take (k, J) mean and variance rows; n_obs is free."""
        R = np.ascontiguousarray(np.asarray(R, dtype=np.float64))
        if R.ndim != 2 or R.shape[0] != R.shape[1]:
            raise ValueError("gp_proj_set: R has shape %s, expected (k, k)" % (R.shape,))
        a0 = np.ascontiguousarray(np.asarray(a0, dtype=np.float64).reshape(-1))
        if a0.shape != (R.shape[0],):
            raise ValueError("gp_proj_set: a0 has %d values, expected %d" % (a0.size, R.shape[0]))
        d = GpProjDesc(C.sizeof(GpProjDesc), R.shape[0], 1 if logdet else 0, R.ctypes.data if R.size else None,
                       a0.ctypes.data if a0.size else None, float(c_perp), float(half_logdet_gamma))
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_gp_proj_set(self._h, C.byref(d)))

    def gp_predict(self, X, nugget=True, var=True, out=None):
        """(mean, var) float64 device tensors (n_gp, J) of the installed GPs at the columns of X (cesx_gp_predict);
        var=False: the mean-only mode, var is None.  ``out``: a (mean, var) pair to write into."""
        mean, v = out if out is not None else (None, None)
        if mean is None:
            mean = torch.empty((self.gp_n, self.J), dtype=torch.float64, device=self.device)
        if var and v is None:
            v = torch.empty((self.gp_n, self.J), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_gp_predict(self._h, X.data_ptr(), mean.data_ptr(), v.data_ptr() if var else None,
                                                 1 if nugget else 0, self._stream()))
        self._keep_gp = (X, mean, v)
        return mean, (v if var else None)

    def gp_start(self, mode, U, mean, var=None):
        """phi of the current states U from their GP rows in likelihood mode ``mode`` (GP_MODES); counters cleared."""
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_gp_start(self._h, GP_MODES[mode], U.data_ptr(), mean.data_ptr(),
                                               None if var is None else var.data_ptr(), self._stream()))
        self._keep_gp_s = (U, mean, var)

    def gp_accept(self, mode, step_index, U, P, mean, var=None, logu=None):
        """phi(P) from its GP rows, the test log u < phi(U) - phi(P), U := P on the accepted columns (cesx_gp_accept)."""
        if logu is not None:
            assert logu.dtype == torch.float64 and logu.numel() == self.J and logu.is_contiguous()
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_gp_accept(self._h, GP_MODES[mode], int(step_index), U.data_ptr(), P.data_ptr(),
                                                mean.data_ptr(), None if var is None else var.data_ptr(),
                                                None if logu is None else logu.data_ptr(), self._stream()))
        self._keep_gp_a = (U, P, mean, var, logu)

    def gp_run(self, mode, step_index, n_steps, U, stride=1, trace=None, xi=None, logu=None, nugget=True):
        """``n_steps`` Metropolis steps of every chain on the installed emulator in one launch (cesx_gp_run), likelihood
        mode ``mode`` of GP_MODES ('gamma', 'var', 'gamma_var'): ``U`` (p, J) is advanced in place, the engine's phi,
        counters and step count follow.  ``trace`` (n_steps // stride, p, J) engine dtype, or None; ``xi`` (n_steps, p, J)
        engine dtype and ``logu`` (n_steps, J) float64, or None for the device draws of steps ``step_index`` ..
        ``step_index + n_steps - 1``; ``nugget`` as in ``gp_predict``.  An emulator whose tile does not fit in LDS raises
        ``CesxError`` with code EUNSUPPORTED."""
        n_steps, stride = int(n_steps), int(stride)
        for name, t, shape, dt in (("U", U, (self.p, self.J), self.torch_dtype),
                                   ("trace", trace, (max(n_steps, 0) // max(stride, 1), self.p, self.J), self.torch_dtype),
                                   ("xi", xi, (n_steps, self.p, self.J), self.torch_dtype),
                                   ("logu", logu, (n_steps, self.J), torch.float64)):
            if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda):
                raise ValueError("gp_run: %s must be a contiguous %s tensor of shape %s" % (name, dt, shape))
        with torch.cuda.device(self.device):
            rc = self.lib.cesx_gp_run(self._h, GP_MODES[mode], int(step_index), n_steps, stride, 1 if nugget else 0,
                                      U.data_ptr(), None if trace is None or trace.numel() == 0 else trace.data_ptr(),
                                      None if xi is None else xi.data_ptr(),
                                      None if logu is None else logu.data_ptr(), self._stream())
            if rc == EUNSUPPORTED:            # (the LDS limit, not the reference's missing LM_procedure of _check)
                raise CesxError(rc, self.lib.cesx_last_error(self._h).decode())
            self._check(rc)
        self._keep_gp_run = (U, trace, xi, logu)

    def gp_predict_grad(self, X, nugget=True, var=True, out=None):
        """(mean, var, dmean, dvar): ``gp_predict`` with the gradients of every GP row with respect to x, float64 device
        tensors (n_gp, p, J) (cesx_gp_predict_grad); mean and var are ``gp_predict``'s bit for bit.  var=False: the
        mean-only mode, var and dvar are None.  ``out``: a (mean, var, dmean, dvar) tuple to write into.  An emulator with
        a Matern12 GP raises ``CesxError`` with code EUNSUPPORTED."""
        mean, v, dm, dv = out if out is not None else (None, None, None, None)
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self.device)      # noqa: E731
        mean = new(self.gp_n, self.J) if mean is None else mean
        dm = new(self.gp_n, self.p, self.J) if dm is None else dm
        if var:
            v = new(self.gp_n, self.J) if v is None else v
            dv = new(self.gp_n, self.p, self.J) if dv is None else dv
        with torch.cuda.device(self.device):
            rc = self.lib.cesx_gp_predict_grad(self._h, X.data_ptr(), mean.data_ptr(), v.data_ptr() if var else None,
                                               dm.data_ptr(), dv.data_ptr() if var else None, 1 if nugget else 0,
                                               self._stream())
            if rc == EUNSUPPORTED:            # (Matern12, not the reference's missing LM_procedure of _check)
                raise CesxError(rc, self.lib.cesx_last_error(self._h).decode())
            self._check(rc)
        self._keep_gp_g = (X, mean, v, dm, dv)
        return mean, (v if var else None), dm, (dv if var else None)

    def gp_langevin_start(self, mode, U, mean, var, dmean, dvar):
        """phi and g = S^T grad phi of the current states U from their GP rows and gradients (``gp_predict_grad`` at U) in
        likelihood mode ``mode`` ('gamma', 'var', 'gamma_var'); counters cleared (cesx_gp_langevin_start).  Mode 'proj': the
        projected Sigma of ``gp_proj_set``, rows (k, J) and gradients (k, p, J) (cesx_gp_proj_langevin_start)."""
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        with torch.cuda.device(self.device):
            if mode == "proj":
                self._check_proj(self.lib.cesx_gp_proj_langevin_start(self._h, U.data_ptr(), ptr(mean), ptr(var), ptr(dmean),
                                                                      ptr(dvar), self._stream()))
            else:
                self._check(self.lib.cesx_gp_langevin_start(self._h, GP_MODES[mode], U.data_ptr(), ptr(mean), ptr(var), ptr(dmean),
                                                            ptr(dvar), self._stream()))
        self._keep_lv_s = (U, mean, var, dmean, dvar)

    def gp_langevin_propose(self, step_index, U, xi=None, out=None):
        """P = U + S (xi - g(U) / 2) (cesx_gp_langevin_propose); xi None: drawn on device in the MH counter domain of
        step_index.  The engine keeps the block for ``gp_langevin_accept``."""
        out = self.empty(self.p) if out is None else out
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_gp_langevin_propose(self._h, int(step_index), U.data_ptr(),
                                                          None if xi is None else xi.data_ptr(), out.data_ptr(), self._stream()))
        self._keep_lv_p = (U, xi, out)
        return out

    def gp_langevin_accept(self, mode, step_index, U, P, mean, var, dmean, dvar, logu=None):
        """phi(P) and g(P) from the rows and gradients at P, the test with the Langevin correction, U := P on the accepted
        columns (cesx_gp_langevin_accept); logu as in ``gp_accept``."""
        if logu is not None:
            assert logu.dtype == torch.float64 and logu.numel() == self.J and logu.is_contiguous()
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        with torch.cuda.device(self.device):
            if mode == "proj":
                self._check_proj(self.lib.cesx_gp_proj_langevin_accept(self._h, int(step_index), U.data_ptr(), P.data_ptr(), ptr(mean),
                                                                       ptr(var), ptr(dmean), ptr(dvar), ptr(logu), self._stream()))
            else:
                self._check(self.lib.cesx_gp_langevin_accept(self._h, GP_MODES[mode], int(step_index), U.data_ptr(), P.data_ptr(),
                                                             ptr(mean), ptr(var), ptr(dmean), ptr(dvar), ptr(logu), self._stream()))
        self._keep_lv_a = (U, P, mean, var, dmean, dvar, logu)

    def _check_proj(self, rc):
        """``_check`` for the cesx_gp_proj_* calls: EUNSUPPORTED is a Matern12 image (not the reference's missing LM_procedure)."""
        if rc == EUNSUPPORTED:
            raise CesxError(rc, self.lib.cesx_last_error(self._h).decode())
        self._check(rc)

    def gp_proj_coef(self, mean, var, out=None):
        """(phi_data (J,), a (k, J), b (k, J)), float64 device tensors: the data term of phi in mode 'proj' and the gradient
        coefficients a_t = d phi / d m_t, b_t = d phi / d v_t of the projected Sigma from the rows ``mean``, ``var`` (k, J)
        (cesx_gp_proj_coef; the descriptor of ``gp_proj_set``).  ``out``: a (phi, a, b) tuple to write into."""
        k = mean.shape[0]
        if k != getattr(self, "gp_n", k):         # (the kernel reads the descriptor's k rows: n_gp == k is the C side's check)
            raise ValueError("gp_proj_coef: %d rows for the emulator's n_gp = %d" % (k, self.gp_n))
        if out is None:
            out = (torch.empty(self.J, dtype=torch.float64, device=self.device),
                   torch.empty((k, self.J), dtype=torch.float64, device=self.device),
                   torch.empty((k, self.J), dtype=torch.float64, device=self.device))
        for name, t, shape in (("mean", mean, (k, self.J)), ("var", var, (k, self.J)), ("phi", out[0], (self.J,)),
                               ("a", out[1], (k, self.J)), ("b", out[2], (k, self.J))):
            if t is None or t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
                raise ValueError("gp_proj_coef: %s must be a contiguous float64 device tensor of shape %s" % (name, shape))
        with torch.cuda.device(self.device):
            self._check_proj(self.lib.cesx_gp_proj_coef(self._h, mean.data_ptr(), var.data_ptr(), out[0].data_ptr(),
                                                        out[1].data_ptr(), out[2].data_ptr(), self._stream()))
        self._keep_gp_pc = (mean, var, out)
        return out

    # -- GP training: the batched likelihood and gradient (include/cesx.h, cesx_gpfit_*; ces_amd/emulate.py drives it) --
    def gpfit_set(self, X, Y, family, ard=True, mean="zero"):
        """Install a fit problem: training inputs X (J_t, p) shared by the GPs, targets Y (n_gp, J_t), kernel family 0..3,
        ARD, mean kind 'zero' / 'constant' / 'linear' (cesx_gpfit_set).  Returns the parameters per GP."""
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
        Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64))
        if X.ndim != 2 or X.shape[1] != self.p:
            raise ValueError("gpfit_set: X has shape %s, expected (J_t, %d)" % (X.shape, self.p))
        if Y.ndim != 2 or Y.shape[1] != X.shape[0]:
            raise ValueError("gpfit_set: Y has shape %s, expected (n_gp, %d)" % (Y.shape, X.shape[0]))
        if mean not in GPFIT_MEANS:
            raise ValueError("gpfit_set: unknown mean kind %r" % (mean,))
        d = GpFitDesc(C.sizeof(GpFitDesc), Y.shape[0], X.shape[0], int(family), 1 if ard else 0, GPFIT_MEANS[mean],
                      X.ctypes.data, Y.ctypes.data)
        self.gpfit_n = self.gpfit_ntheta = 0
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_gpfit_set(self._h, C.byref(d)))
        self.gpfit_n, self.gpfit_Jt = int(Y.shape[0]), int(X.shape[0])
        self.gpfit_ntheta = int(self.lib.cesx_gpfit_ntheta(self._h))
        return self.gpfit_ntheta

    def gpfit_eval(self, idx, theta):
        """(lml (k,), grad (k, n_theta), status (k,) int32: OK or ENOTPD) of the GPs ``idx`` at the natural parameters
        ``theta`` (k, n_theta) in ``GPR._get()`` order, one batched evaluation (cesx_gpfit_eval)."""
        if not getattr(self, "gpfit_n", 0):
            raise CesxError(ESTATE, "gpfit_eval: gpfit_set has not been called")
        idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int32).reshape(-1))
        theta = np.ascontiguousarray(np.asarray(theta, dtype=np.float64))
        k, nt = idx.size, self.gpfit_ntheta
        if theta.shape != (k, nt):
            raise ValueError("gpfit_eval: theta has shape %s, expected %s" % (theta.shape, (k, nt)))
        lml, grad, status = np.empty(k), np.empty((k, nt)), np.empty(k, dtype=np.int32)
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_gpfit_eval(self._h, k, idx.ctypes.data, theta.ctypes.data, lml.ctypes.data,
                                                 grad.ctypes.data, status.ctypes.data, self._stream()))
        return lml, grad, status

    def gpfit_factors(self, i):
        """(alpha (J_t,), L^{-1} (J_t, J_t)) of GP ``i`` as of its last evaluation, on the host (cesx_gpfit_factors)."""
        if not getattr(self, "gpfit_n", 0):
            raise CesxError(ESTATE, "gpfit_factors: gpfit_set has not been called")
        alpha, Li = np.empty(self.gpfit_Jt), np.empty((self.gpfit_Jt, self.gpfit_Jt))
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_gpfit_factors(self._h, int(i), alpha.ctypes.data, Li.ctypes.data))
        return alpha, Li

    # -- Darcy forward map over the columns (include/cesx.h, cesx_darcy_*; ces_amd/darcy.py builds the descriptor) --
    def darcy_set(self, desc):
        """Install a Darcy map: ``desc`` as ``ces_amd.darcy.model.device_descriptor`` returns it (the engine keeps its own
        copy): cesx_darcy_set, or cesx_darcy_set_streamed with ``desc['max_workgroups']`` when ``desc['solver']`` is
        ``'streamed'``.  Returns the token that identifies the installed map."""
        K = int(desc["K"])
        mats = {k: np.ascontiguousarray(np.asarray(desc[k], dtype=np.float64)) for k in ("coef", "D", "S", "R")}
        for k, a in mats.items():
            if a.shape != (K, K):
                raise ValueError("darcy_set: %s has shape %s, expected %s" % (k, a.shape, (K, K)))
        scatter = np.ascontiguousarray(np.asarray(desc["scatter"], dtype=np.int32).reshape(-1))
        obs = np.ascontiguousarray(np.asarray(desc["obs_index"], dtype=np.int32).reshape(-1))
        d = DarcyDesc(C.sizeof(DarcyDesc), K, scatter.size, obs.size, mats["coef"].ctypes.data, scatter.ctypes.data,
                      mats["D"].ctypes.data, mats["S"].ctypes.data, mats["R"].ctypes.data, obs.ctypes.data)
        with torch.cuda.device(self.device):
            solver = desc.get("solver", "resident")
            if solver == "streamed":
                self._check(self.lib.cesx_darcy_set_streamed(self._h, C.byref(d), int(desc.get("max_workgroups", 0))))
            elif solver == "resident":
                self._check(self.lib.cesx_darcy_set(self._h, C.byref(d)))
            else:
                raise ValueError("darcy_set: solver %r is neither 'resident' nor 'streamed'" % (solver,))
        self._darcy_token = object()
        return self._darcy_token

    def darcy_workspace_bytes(self):
        """Bytes of HBM workspace the installed Darcy map owns (cesx_darcy_workspace_bytes): 0 unless it is a streamed one."""
        return int(self.lib.cesx_darcy_workspace_bytes(self._h))

    def darcy_grad(self, U, out=None, status=None):
        """(G (n_obs, J), phi_d (J,), d (p, J)), float64 device tensors: the installed resident Darcy map of the columns of U, the
        data misfit 1/2 r^T Gamma^{-1} r of ``set_problem``'s y and Gamma and its gradient, by one adjoint solve per particle
        (cesx_darcy_grad).  ``out``: such a tuple.  ``status``: an int32 device tensor (J,) for ``darcy_apply``'s status words.
        Nothing is read back and nothing raised for a particle: one whose system is singular or not finite has NaN in all three."""
        G, phid, d = out if out is not None else (None, None, None)
        G = torch.empty((self.n_obs, self.J), dtype=torch.float64, device=self.device) if G is None else G
        phid = torch.empty((self.J,), dtype=torch.float64, device=self.device) if phid is None else phid
        d = torch.empty((self.p, self.J), dtype=torch.float64, device=self.device) if d is None else d
        for name, t, shape, dt in (("U", U, (self.p, self.J), self.torch_dtype), ("G", G, (self.n_obs, self.J), torch.float64),
                                   ("phi_d", phid, (self.J,), torch.float64), ("d", d, (self.p, self.J), torch.float64),
                                   ("status", status, (self.J,), torch.int32)):
            if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda):
                raise ValueError("darcy_grad: %s must be a contiguous %s tensor of shape %s" % (name, dt, shape))
        with torch.cuda.device(self.device):
            rc = self.lib.cesx_darcy_grad(self._h, U.data_ptr(), G.data_ptr(), phid.data_ptr(), d.data_ptr(),
                                          None if status is None else status.data_ptr(), self._stream())
            if rc == EUNSUPPORTED:            # (a streamed map, not the reference's missing LM_procedure of _check)
                raise CesxError(rc, self.lib.cesx_last_error(self._h).decode())
            self._check(rc)
        self._keep_darcy_grad = (U, G, phid, d, status)
        return G, phid, d

    def darcy_apply(self, U, out=None):
        """G (n_obs, J) = the installed Darcy map of the columns of U (cesx_darcy_apply).  Raises ``numpy.linalg.LinAlgError``
        naming the first particle whose system is exactly singular, or whose system left fp64's range (exp(theta) overflowed) --
        the outputs of such a particle are NaN; the host map's ``spsolve`` warns and returns NaN or inf there.  Reads the
        per-particle status words: synchronises."""
        out = self.empty(self.n_obs) if out is None else out
        status = self.__dict__.get("_darcy_status")
        if status is None:
            status = self._darcy_status = torch.empty(self.J, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_darcy_apply(self._h, U.data_ptr(), out.data_ptr(), status.data_ptr(), self._stream()))
            self._keep_darcy = (U, out)
            bad = torch.nonzero(status).reshape(-1)
            if bad.numel():
                j = int(bad[0])
                st = int(status[j])
                if st > 0:
                    raise np.linalg.LinAlgError("Darcy forward map: the system of particle %d is singular (zero pivot in "
                                                "column %d)" % (j, st - 1))
                raise np.linalg.LinAlgError("Darcy forward map: the system of particle %d is not finite (NaN or inf in column "
                                            "%d: exp(theta) overflowed?)" % (j, -st - 1))
        return out

    # -- Lorenz '96 forward map over the columns (include/cesx.h, cesx_lorenz_*; ces_amd/models.py builds the descriptor) --
    def l96_set(self, desc):
        """Install a Lorenz '96 map: ``desc`` as ``ces_amd.models.lorenz96.device_descriptor`` returns it (cesx_lorenz_set; the
        engine keeps its own copy).  Returns the token that identifies the installed map."""
        d, t = l96_desc_struct(desc)
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_lorenz_set(self._h, C.byref(d)))
        del t
        self._l96_token = object()
        self._l96_n_state = int(desc["n_slow"]) * (int(desc["n_fast"]) + 1)
        return self._l96_token

    def l96_apply(self, U, W, out=None, W_out=None):
        """(G (n_obs, J) engine dtype, W_out (n_state, J) fp64, info (4, J) int32) of the installed map for the parameter
        columns of ``U`` started from the columns of ``W`` (cesx_lorenz_apply).  ``W_out`` may be ``W``.  Nothing is read back:
        ``info[0]`` holds each particle's status (0, or a key of ``L96_STATUS``; such a particle's outputs are NaN)."""
        ns = self.__dict__.get("_l96_n_state")
        if ns is None:
            raise CesxError(ESTATE, "l96_apply: l96_set has not been called")
        if W.dtype != torch.float64 or tuple(W.shape) != (ns, self.J) or not W.is_contiguous():
            raise ValueError("l96_apply: W must be a contiguous float64 tensor of shape %s" % ((ns, self.J),))
        out = self.empty(self.n_obs) if out is None else out
        W_out = torch.empty((ns, self.J), dtype=torch.float64, device=self.device) if W_out is None else W_out
        if W_out.dtype != torch.float64 or tuple(W_out.shape) != (ns, self.J) or not W_out.is_contiguous():
            raise ValueError("l96_apply: W_out must be a contiguous float64 tensor of shape %s" % ((ns, self.J),))
        info = torch.empty((4, self.J), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_lorenz_apply(self._h, U.data_ptr(), W.data_ptr(), out.data_ptr(), W_out.data_ptr(),
                                                info.data_ptr(), self._stream()))
            self._keep_l96 = (U, W, out, W_out, info)
        return out, W_out, info

    # -- Lorenz '63 forward map over the columns (include/cesx.h, cesx_lorenz_three_*; ces_amd/models.py builds the descriptor) --
    def l63_set(self, desc):
        """Install a Lorenz '63 map: ``desc`` as ``ces_amd.models.lorenz63.device_descriptor`` returns it
        (cesx_lorenz_three_set; the engine keeps its own copy).  Returns the token that identifies the installed map."""
        d, t = l63_desc_struct(desc)
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_lorenz_three_set(self._h, C.byref(d)))
        del t
        self._l63_token = object()
        return self._l63_token

    def l63_apply(self, U, W, out=None, W_out=None):
        """(G (9, J) engine dtype, W_out (3, J) fp64, info (4, J) int32) of the installed map for the parameter columns of
        ``U`` started from the columns of ``W`` (cesx_lorenz_three_apply).  ``W_out`` may be ``W``.  Nothing is read back:
        ``info[0]`` holds each particle's status (0, or a key of ``L63_STATUS``; such a particle's outputs are NaN)."""
        if self.__dict__.get("_l63_token") is None:
            raise CesxError(ESTATE, "l63_apply: l63_set has not been called")
        if W.dtype != torch.float64 or tuple(W.shape) != (3, self.J) or not W.is_contiguous():
            raise ValueError("l63_apply: W must be a contiguous float64 tensor of shape %s" % ((3, self.J),))
        out = self.empty(self.n_obs) if out is None else out
        W_out = torch.empty((3, self.J), dtype=torch.float64, device=self.device) if W_out is None else W_out
        if W_out.dtype != torch.float64 or tuple(W_out.shape) != (3, self.J) or not W_out.is_contiguous():
            raise ValueError("l63_apply: W_out must be a contiguous float64 tensor of shape %s" % ((3, self.J),))
        info = torch.empty((4, self.J), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_lorenz_three_apply(self._h, U.data_ptr(), W.data_ptr(), out.data_ptr(), W_out.data_ptr(),
                                                         info.data_ptr(), self._stream()))
            self._keep_l63 = (U, W, out, W_out, info)
        return out, W_out, info

    # -- closed-form maps over the columns and their fused chain kernel (include/cesx.h, cesx_map_*, cesx_mh_run_map) --
    def map_set(self, kind, prm=()):
        """Install a closed-form map: ``kind`` a key of ``MAP_KINDS`` ('elliptic': prm (x1, x2); 'banana': prm (a, b);
        'exp': none -- the prologue of ``lineal_log``, for which the (p, J) scratch buffer ``map_scratch`` is allocated
        here, once) (cesx_map_set).  Returns the token that identifies the installed map."""
        if kind not in MAP_KINDS:
            raise ValueError("unknown map kind %r" % (kind,))
        prm = [float(v) for v in prm]
        if len(prm) > 8:
            raise ValueError("map_set: at most 8 parameters")
        d = MapDesc()
        d.struct_bytes, d.kind = C.sizeof(MapDesc), MAP_KINDS[kind]
        for k, v in enumerate(prm):
            d.prm[k] = v
        self._check(self.lib.cesx_map_set(self._h, C.byref(d)))
        if kind == "exp" and self.__dict__.get("map_scratch") is None:
            self.map_scratch = self.empty(self.p)
        self.map_kind = kind
        self._map_token = object()
        return self._map_token

    def map_apply(self, U, out=None):
        """G = the installed map of the columns of ``U`` (cesx_map_apply): (n_obs, J), for 'exp' (p, J), engine dtype."""
        if self.__dict__.get("_map_token") is None:
            raise CesxError(ESTATE, "map_apply: map_set has not been called")
        rows = self.p if self.map_kind == "exp" else self.n_obs
        out = self.empty(rows) if out is None else out
        for name, t, r in (("U", U, self.p), ("out", out, rows)):
            if t.dtype != self.torch_dtype or tuple(t.shape) != (r, self.J) or not t.is_contiguous() or not t.is_cuda:
                raise ValueError("map_apply: %s must be a contiguous %s tensor of shape %s" % (name, self.torch_dtype, (r, self.J)))
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_map_apply(self._h, U.data_ptr(), out.data_ptr(), self._stream()))
        self._keep_map = (U, out)
        return out

    def mh_run_map(self, step_index, n_steps, U, stride=1, trace=None, xi=None, logu=None):
        """``n_steps`` Metropolis steps of every chain in one launch with the installed map of a fused kind
        (cesx_mh_run_map): ``U`` (p, J) is advanced in place, the engine's phi, counters and step count follow.
        ``trace`` (n_steps // stride, p, J) engine dtype, or None; ``xi`` (n_steps, p, J) engine dtype and ``logu``
        (n_steps, J) float64, or None for the device draws of steps ``step_index`` .. ``step_index + n_steps - 1``."""
        n_steps, stride = int(n_steps), int(stride)
        for name, t, shape, dt in (("U", U, (self.p, self.J), self.torch_dtype),
                                   ("trace", trace, (max(n_steps, 0) // max(stride, 1), self.p, self.J), self.torch_dtype),
                                   ("xi", xi, (n_steps, self.p, self.J), self.torch_dtype),
                                   ("logu", logu, (n_steps, self.J), torch.float64)):
            if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda):
                raise ValueError("mh_run_map: %s must be a contiguous %s tensor of shape %s" % (name, dt, shape))
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_run_map(self._h, int(step_index), n_steps, stride, U.data_ptr(),
                                                 None if trace is None or trace.numel() == 0 else trace.data_ptr(),
                                                 None if xi is None else xi.data_ptr(),
                                                 None if logu is None else logu.data_ptr(), self._stream()))
        self._keep_mh_run = (U, trace, xi, logu)

    # -- the Langevin step on a closed-form map and its Jacobian (include/cesx.h, cesx_map_jac, cesx_mh_langevin_*) --
    def map_jac(self, U, out=None):
        """(G, DG): the installed map of the columns of ``U`` and its Jacobian ``DG[i][q] = dG_i / du_q``, float64 device
        tensors (n_obs, J) and (n_obs, p, J) whatever the engine dtype (cesx_map_jac).  ``out``: a (G, DG) tuple to write
        into.  The 'exp' map of ``lineal_log`` raises ``CesxError`` with code EUNSUPPORTED."""
        if self.__dict__.get("_map_token") is None:
            raise CesxError(ESTATE, "map_jac: map_set has not been called")
        G, DG = out if out is not None else (None, None)
        G = torch.empty((self.n_obs, self.J), dtype=torch.float64, device=self.device) if G is None else G
        DG = torch.empty((self.n_obs, self.p, self.J), dtype=torch.float64, device=self.device) if DG is None else DG
        for name, t, shape, dt in (("U", U, (self.p, self.J), self.torch_dtype), ("G", G, (self.n_obs, self.J), torch.float64),
                                   ("DG", DG, (self.n_obs, self.p, self.J), torch.float64)):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
                raise ValueError("map_jac: %s must be a contiguous %s tensor of shape %s" % (name, dt, shape))
        with torch.cuda.device(self.device):
            rc = self.lib.cesx_map_jac(self._h, U.data_ptr(), G.data_ptr(), DG.data_ptr(), self._stream())
            if rc == EUNSUPPORTED:            # (the 'exp' map, not the reference's missing LM_procedure of _check)
                raise CesxError(rc, self.lib.cesx_last_error(self._h).decode())
            self._check(rc)
        self._keep_map_jac = (U, G, DG)
        return G, DG

    def mh_langevin_start(self, U, G, DG):
        """phi (with the prior term) and g = S^T grad phi of the current states U from their forward map ``G`` (n_obs, J)
        and its Jacobian ``DG`` (n_obs, p, J), float64 (``map_jac`` at U); counters cleared (cesx_mh_langevin_start)."""
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_langevin_start(self._h, U.data_ptr(), G.data_ptr(), DG.data_ptr(), self._stream()))
        self._keep_lv_s = (U, G, DG)

    def mh_langevin_propose(self, step_index, U, xi=None, out=None):
        """P = U + S (xi - g(U) / 2) (cesx_mh_langevin_propose); xi None: drawn on device in the MH counter domain of
        step_index.  The engine keeps the block for ``mh_langevin_accept``."""
        out = self.empty(self.p) if out is None else out
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_langevin_propose(self._h, int(step_index), U.data_ptr(),
                                                          None if xi is None else xi.data_ptr(), out.data_ptr(), self._stream()))
        self._keep_lv_p = (U, xi, out)
        return out

    def mh_langevin_accept(self, step_index, U, P, G, DG, logu=None):
        """phi(P) and g(P) from the map ``G`` and the Jacobian ``DG`` at P, the test with the Langevin correction, U := P on
        the accepted columns (cesx_mh_langevin_accept); logu as in ``mh_accept``."""
        if logu is not None:
            assert logu.dtype == torch.float64 and logu.numel() == self.J and logu.is_contiguous()
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_langevin_accept(self._h, int(step_index), U.data_ptr(), P.data_ptr(), G.data_ptr(),
                                                         DG.data_ptr(), None if logu is None else logu.data_ptr(), self._stream()))
        self._keep_lv_a = (U, P, G, DG, logu)

    def mh_langevin_run_map(self, step_index, n_steps, U, stride=1, trace=None, xi=None, logu=None):
        """``n_steps`` Langevin steps of every chain in one launch with the installed map of a fused kind
        (cesx_mh_langevin_run_map): ``mh_run_map`` under a Langevin proposal, after ``mh_langevin_start``; the engine's phi,
        g, counters and step count follow.  The arguments are ``mh_run_map``'s."""
        n_steps, stride = int(n_steps), int(stride)
        for name, t, shape, dt in (("U", U, (self.p, self.J), self.torch_dtype),
                                   ("trace", trace, (max(n_steps, 0) // max(stride, 1), self.p, self.J), self.torch_dtype),
                                   ("xi", xi, (n_steps, self.p, self.J), self.torch_dtype),
                                   ("logu", logu, (n_steps, self.J), torch.float64)):
            if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda):
                raise ValueError("mh_langevin_run_map: %s must be a contiguous %s tensor of shape %s" % (name, dt, shape))
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_langevin_run_map(self._h, int(step_index), n_steps, stride, U.data_ptr(),
                                                          None if trace is None or trace.numel() == 0 else trace.data_ptr(),
                                                          None if xi is None else xi.data_ptr(),
                                                          None if logu is None else logu.data_ptr(), self._stream()))
        self._keep_mh_run = (U, trace, xi, logu)

    # -- leapfrog HMC under a Langevin proposal (include/cesx.h, cesx_mh_hmc_* / cesx_gp_hmc_*): after mh_langevin_start / gp_langevin_start --
    def mh_hmc_begin(self, step_index, U, xi=None, out=None):
        """r = xi - g(U) / 2 and the first leapfrog position Q = U + S r (cesx_mh_hmc_begin; the map's and the emulator's);
        xi None: drawn on device in the MH counter domain of step_index.  The engine keeps the block and r."""
        out = self.empty(self.p) if out is None else out
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_hmc_begin(self._h, int(step_index), U.data_ptr(),
                                                   None if xi is None else xi.data_ptr(), out.data_ptr(), self._stream()))
        self._keep_hm_b = (U, xi, out)
        return out

    def mh_hmc_leap(self, Q, G, DG):
        """phi(Q), g(Q) from the map ``G`` and the Jacobian ``DG`` at Q (``map_jac``), the full kick r = r - g(Q) and the next
        position Q = Q + S r in place (cesx_mh_hmc_leap)."""
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_hmc_leap(self._h, Q.data_ptr(), G.data_ptr(), DG.data_ptr(), self._stream()))
        self._keep_hm_l = (Q, G, DG)

    def mh_hmc_accept(self, step_index, U, Q, G, DG, logu=None):
        """phi(Q), g(Q) at the last position, the half kick, the test log u < phi(U) - phi(Q) + |xi|^2 / 2 - |r|^2 / 2, U := Q on
        the accepted columns (cesx_mh_hmc_accept); logu as in ``mh_accept``."""
        if logu is not None:
            assert logu.dtype == torch.float64 and logu.numel() == self.J and logu.is_contiguous()
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_hmc_accept(self._h, int(step_index), U.data_ptr(), Q.data_ptr(), G.data_ptr(),
                                                    DG.data_ptr(), None if logu is None else logu.data_ptr(), self._stream()))
        self._keep_hm_a = (U, Q, G, DG, logu)

    def gp_hmc_leap(self, mode, Q, mean, var, dmean, dvar):
        """``mh_hmc_leap`` on the GP rows and gradients at Q (``gp_predict_grad``) in likelihood mode ``mode`` (cesx_gp_hmc_leap)."""
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        with torch.cuda.device(self.device):
            if mode == "proj":                   # (cesx_gp_proj_hmc_leap: the projected Sigma of ``gp_proj_set``)
                self._check_proj(self.lib.cesx_gp_proj_hmc_leap(self._h, Q.data_ptr(), ptr(mean), ptr(var), ptr(dmean), ptr(dvar),
                                                                self._stream()))
            else:
                self._check(self.lib.cesx_gp_hmc_leap(self._h, GP_MODES[mode], Q.data_ptr(), ptr(mean), ptr(var), ptr(dmean),
                                                      ptr(dvar), self._stream()))
        self._keep_hm_l = (Q, mean, var, dmean, dvar)

    def gp_hmc_accept(self, mode, step_index, U, Q, mean, var, dmean, dvar, logu=None):
        """``mh_hmc_accept`` on the GP rows and gradients at the last Q in likelihood mode ``mode`` (cesx_gp_hmc_accept)."""
        if logu is not None:
            assert logu.dtype == torch.float64 and logu.numel() == self.J and logu.is_contiguous()
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        with torch.cuda.device(self.device):
            if mode == "proj":                   # (cesx_gp_proj_hmc_accept)
                self._check_proj(self.lib.cesx_gp_proj_hmc_accept(self._h, int(step_index), U.data_ptr(), Q.data_ptr(), ptr(mean),
                                                                  ptr(var), ptr(dmean), ptr(dvar), ptr(logu), self._stream()))
            else:
                self._check(self.lib.cesx_gp_hmc_accept(self._h, GP_MODES[mode], int(step_index), U.data_ptr(), Q.data_ptr(),
                                                        ptr(mean), ptr(var), ptr(dmean), ptr(dvar), ptr(logu), self._stream()))
        self._keep_hm_a = (U, Q, mean, var, dmean, dvar, logu)

    def mh_hmc_run_map(self, step_index, n_steps, leapfrog, U, stride=1, trace=None, xi=None, logu=None):
        """``n_steps`` HMC steps of ``leapfrog`` positions each of every chain in one launch with the installed map of a fused
        kind (cesx_mh_hmc_run_map; ``n_steps * leapfrog <= 4096``), after ``mh_langevin_start``; the engine's phi, g, counters
        and step count follow.  The other arguments are ``mh_run_map``'s."""
        n_steps, stride, leapfrog = int(n_steps), int(stride), int(leapfrog)
        for name, t, shape, dt in (("U", U, (self.p, self.J), self.torch_dtype),
                                   ("trace", trace, (max(n_steps, 0) // max(stride, 1), self.p, self.J), self.torch_dtype),
                                   ("xi", xi, (n_steps, self.p, self.J), self.torch_dtype),
                                   ("logu", logu, (n_steps, self.J), torch.float64)):
            if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda):
                raise ValueError("mh_hmc_run_map: %s must be a contiguous %s tensor of shape %s" % (name, dt, shape))
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_hmc_run_map(self._h, int(step_index), n_steps, leapfrog, stride, U.data_ptr(),
                                                     None if trace is None or trace.numel() == 0 else trace.data_ptr(),
                                                     None if xi is None else xi.data_ptr(),
                                                     None if logu is None else logu.data_ptr(), self._stream()))
        self._keep_mh_run = (U, trace, xi, logu)

    # -- pooled step-size adaptation of the leapfrog step (include/cesx.h, cesx_mh_adapt_*): after mh_set_proposal('langevin' / 'hmc') --
    def mh_adapt_set(self, n_steps, target, gain=2.0, kappa=0.75):
        """Arm the handle for ``n_steps`` adaptation steps towards the mean acceptance ``target`` (cesx_mh_adapt_set): until
        the next ``mh_set_proposal`` the ``mh_hmc_*`` / ``gp_hmc_*`` steps run at e S and every accept updates e on the device."""
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_adapt_set(self._h, int(n_steps), float(target), float(gain), float(kappa)))

    def mh_grad_source(self, source):
        """Where ``mh_langevin_start`` / ``_accept`` and ``mh_hmc_leap`` / ``_accept`` take the data term of grad phi from
        (cesx_mh_grad_source): ``'jacobian'`` -- their ``DG`` is the (n_obs, p, J) image, the default after every
        ``mh_set_proposal`` -- or ``'ready'`` -- ``DG`` is the (p, J) float64 block d of ``darcy_grad`` at the same states."""
        if source not in GRAD_SOURCES:
            raise ValueError("mh_grad_source: %r is neither 'jacobian' nor 'ready'" % (source,))
        with torch.cuda.device(self.device):
            rc = self.lib.cesx_mh_grad_source(self._h, GRAD_SOURCES[source])
            if rc == EUNSUPPORTED:            # (p > 256, not the reference's missing LM_procedure of _check)
                raise CesxError(rc, self.lib.cesx_last_error(self._h).decode())
            self._check(rc)

    def mh_adapt_read(self):
        """``dict(multiplier, steps, history (steps, 2))`` of the adaptation phase: the averaged multiplier, the steps made and
        per step (e_t, mean acceptance probability) (cesx_mh_adapt_read; synchronises)."""
        mult, done = C.c_double(0.0), C.c_int32(0)
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_adapt_read(self._h, C.byref(mult), C.byref(done), None))
            hist = np.zeros((int(done.value), 2), dtype=np.float64)      # (sized by the count the engine reports; steps are made by this thread alone)
            if done.value:
                self._check(self.lib.cesx_mh_adapt_read(self._h, C.byref(mult), C.byref(done), _dptr(hist)))
        return dict(multiplier=float(mult.value), steps=int(done.value), history=hist)

    # -- the Langevin step on a linear map: the gradient as update launches (include/cesx.h, cesx_mh_langevin_lineal_*) --
    def _lvlin_check(self, who, tensors):
        for name, t, rows, dt in tensors:
            if t is not None and (t.dtype != dt or tuple(t.shape) != (rows, self.J) or not t.is_contiguous() or not t.is_cuda):
                raise ValueError("%s: %s must be a contiguous %s tensor of shape %s" % (who, name, dt, (rows, self.J)))

    def mh_langevin_lineal_set(self, A, b=None, exp_params=False):
        """Form and upload the gradient images of the linear map ``A X + b`` (``exp_params``: ``A exp(X) + b``) for the
        installed problem and Langevin proposal (cesx_mh_langevin_lineal_set): ``A`` (n_obs, p), ``b`` None, a scalar or
        (n_obs,).  ``set_problem`` and ``mh_set_proposal`` drop the images."""
        A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
        if A.shape != (self.n_obs, self.p):
            raise ValueError("mh_langevin_lineal_set: A must be (n_obs, p) = %s, got %s" % ((self.n_obs, self.p), A.shape))
        if b is not None:
            b = np.asarray(b, dtype=np.float64)
            if b.ndim > 1 or (b.ndim == 1 and b.shape[0] != self.n_obs):
                raise ValueError("mh_langevin_lineal_set: b must be None, a scalar or (n_obs,), got %s" % (b.shape,))
            b = np.ascontiguousarray(np.broadcast_to(b, (self.n_obs,)))
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_langevin_lineal_set(self._h, _dptr(A), None if b is None else _dptr(b), int(bool(exp_params))))

    def mh_langevin_lineal_start(self, U, G):
        """phi (with the prior term) and g = S^T grad phi of the current states ``U`` (p, J) from their forward map ``G``
        (n_obs, J), both engine dtype; counters cleared (cesx_mh_langevin_lineal_start)."""
        self._lvlin_check("mh_langevin_lineal_start", (("U", U, self.p, self.torch_dtype), ("G", G, self.n_obs, self.torch_dtype)))
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_langevin_lineal_start(self._h, U.data_ptr(), G.data_ptr(), self._stream()))
        self._keep_ll_s = (U, G)

    def mh_langevin_lineal_propose(self, step_index, U, xi=None, out=None):
        """P = U + S (xi - g(U) / 2) (cesx_mh_langevin_lineal_propose); xi None: drawn on device in the MH counter domain
        of step_index.  The engine keeps the block for ``mh_langevin_lineal_accept``."""
        out = self.empty(self.p) if out is None else out
        self._lvlin_check("mh_langevin_lineal_propose", (("U", U, self.p, self.torch_dtype), ("xi", xi, self.p, self.torch_dtype),
                                                         ("out", out, self.p, self.torch_dtype)))
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_langevin_lineal_propose(self._h, int(step_index), U.data_ptr(),
                                                                 None if xi is None else xi.data_ptr(), out.data_ptr(), self._stream()))
        self._keep_ll_p = (U, xi, out)
        return out

    def mh_langevin_lineal_accept(self, step_index, U, P, GP, logu=None):
        """phi(P) and g(P) from the map ``GP`` at P, the test with the Langevin correction, U := P and g := g(P) on the
        accepted columns (cesx_mh_langevin_lineal_accept); logu as in ``mh_accept``."""
        self._lvlin_check("mh_langevin_lineal_accept", (("U", U, self.p, self.torch_dtype), ("P", P, self.p, self.torch_dtype),
                                                        ("GP", GP, self.n_obs, self.torch_dtype)))
        if logu is not None and (logu.dtype != torch.float64 or logu.numel() != self.J or not logu.is_contiguous() or not logu.is_cuda):
            raise ValueError("mh_langevin_lineal_accept: logu must be a contiguous float64 device tensor of J values")
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_langevin_lineal_accept(self._h, int(step_index), U.data_ptr(), P.data_ptr(), GP.data_ptr(),
                                                                None if logu is None else logu.data_ptr(), self._stream()))
        self._keep_ll_a = (U, P, GP, logu)

    def mh_langevin_lineal_g(self):
        """The chains' g = S^T grad phi, float64 (p, J) on the host (cesx_mh_langevin_lineal_g; synchronises)."""
        buf = np.zeros((self.p, self.J), dtype=np.float64)
        self._check(self.lib.cesx_mh_langevin_lineal_g(self._h, _dptr(buf)))
        return buf

    # -- the leapfrog step on a linear map (include/cesx.h, cesx_mh_hmc_lineal_*): after mh_langevin_lineal_start --
    def mh_hmc_lineal_begin(self, step_index, U, xi=None, out=None):
        """r = xi - (e / 2) g(U) and the first leapfrog position Q = U + e S r (cesx_mh_hmc_lineal_begin; e = 1 unless the
        handle is armed); xi None: drawn on device in the MH counter domain of step_index.  The engine keeps the block and r."""
        out = self.empty(self.p) if out is None else out
        self._lvlin_check("mh_hmc_lineal_begin", (("U", U, self.p, self.torch_dtype), ("xi", xi, self.p, self.torch_dtype),
                                                  ("out", out, self.p, self.torch_dtype)))
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_hmc_lineal_begin(self._h, int(step_index), U.data_ptr(),
                                                          None if xi is None else xi.data_ptr(), out.data_ptr(), self._stream()))
        self._keep_hl_b = (U, xi, out)
        return out

    def mh_hmc_lineal_leap(self, Q, GQ, out):
        """g(Q) from the map ``GQ`` at Q, the full kick r = r - e g(Q) and the next position ``out`` = Q + e S r
        (cesx_mh_hmc_lineal_leap); ``out`` is another buffer than ``Q``."""
        self._lvlin_check("mh_hmc_lineal_leap", (("Q", Q, self.p, self.torch_dtype), ("GQ", GQ, self.n_obs, self.torch_dtype),
                                                 ("out", out, self.p, self.torch_dtype)))
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_hmc_lineal_leap(self._h, Q.data_ptr(), GQ.data_ptr(), out.data_ptr(), self._stream()))
        self._keep_hl_l = (Q, GQ, out)
        return out

    def mh_hmc_lineal_accept(self, step_index, U, Q, GQ, logu=None):
        """phi(Q) and g(Q) from the map ``GQ`` at the last position, the half kick, the test
        log u < phi(U) - phi(Q) + |xi|^2 / 2 - |r|^2 / 2, U := Q and g := g(Q) on the accepted columns
        (cesx_mh_hmc_lineal_accept); logu as in ``mh_accept``."""
        self._lvlin_check("mh_hmc_lineal_accept", (("U", U, self.p, self.torch_dtype), ("Q", Q, self.p, self.torch_dtype),
                                                   ("GQ", GQ, self.n_obs, self.torch_dtype)))
        if logu is not None and (logu.dtype != torch.float64 or logu.numel() != self.J or not logu.is_contiguous() or not logu.is_cuda):
            raise ValueError("mh_hmc_lineal_accept: logu must be a contiguous float64 device tensor of J values")
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_mh_hmc_lineal_accept(self._h, int(step_index), U.data_ptr(), Q.data_ptr(), GQ.data_ptr(),
                                                           None if logu is None else logu.data_ptr(), self._stream()))
        self._keep_hl_a = (U, Q, GQ, logu)

    # -- streaming summaries of the chains' draws (include/cesx.h, cesx_chain_summary_*) --
    def chain_summary_begin(self, n_draws):
        """Clear the stage for a run of ``n_draws`` draws per chain (cesx_chain_summary_begin); ValueError below 4."""
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_chain_summary_begin(self._h, int(n_draws), self._stream()))

    def chain_summary_add(self, trace):
        """Add the draws of ``trace``, (kept, p, J) or one state (p, J), engine dtype, in order (cesx_chain_summary_add).
        Nothing is copied: the kernels read ``trace`` on the current stream."""
        shape = tuple(trace.shape)
        if (trace.dtype != self.torch_dtype or not trace.is_cuda or not trace.is_contiguous()
                or shape[-2:] != (self.p, self.J) or len(shape) not in (2, 3)):
            raise ValueError("chain_summary_add: trace must be a contiguous %s tensor of shape (kept, %d, %d) or (%d, %d)"
                             % (self.torch_dtype, self.p, self.J, self.p, self.J))
        kept = shape[0] if len(shape) == 3 else 1
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_chain_summary_add(self._h, trace.data_ptr(), kept, self._stream()))
        self._keep_chain_summary = trace

    def chain_summary_read(self, halves=False):
        """The run's raw sums as host fp64 arrays (cesx_chain_summary_read): ``c`` (p,), ``s1`` (p,), ``cc`` (p, p) lower
        triangle, ``within`` (p,), ``between`` (p,); with ``halves`` also ``half_mean`` and ``half_var`` (2, p, J)."""
        p, J = self.p, self.J
        out = dict(c=np.empty(p), s1=np.empty(p), cc=np.empty((p, p)), within=np.empty(p), between=np.empty(p))
        if halves:
            out.update(half_mean=np.empty((2, p, J)), half_var=np.empty((2, p, J)))
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_chain_summary_read(self._h, out["c"].ctypes.data, out["s1"].ctypes.data, out["cc"].ctypes.data,
                                                         out["within"].ctypes.data, out["between"].ctypes.data,
                                                         out["half_mean"].ctypes.data if halves else None,
                                                         out["half_var"].ctypes.data if halves else None, self._stream()))
        self._keep_chain_summary = None
        return out

    # -- streaming marginals of the chains' draws (include/cesx.h, cesx_chain_hist_*) --
    def chain_hist_begin(self, edges1, edges2=None, pairs=None):
        """Start a run of histograms (cesx_chain_hist_begin): ``edges1`` (p, bins + 1) the 1-D edges of every row,
        ``edges2`` (p, bins2d + 1) the 2-D edges (only the rows named in ``pairs`` are read) and ``pairs`` (P, 2) rows
        (i, j), host fp64 / int.  ValueError for a limit of include/cesx.h; the run in hand then goes on."""
        e1 = np.ascontiguousarray(np.asarray(edges1, dtype=np.float64))
        if e1.ndim != 2 or e1.shape[0] != self.p:
            raise ValueError("chain_hist_begin: edges1 must have shape (%d, bins + 1), got %s" % (self.p, e1.shape))
        pr = np.zeros((0, 2), dtype=np.int32) if pairs is None else np.asarray(pairs)
        if pr.size == 0:
            pr = pr.reshape(0, 2)
        if pr.ndim != 2 or pr.shape[1] != 2 or (pr.size and not np.issubdtype(pr.dtype, np.integer)):
            raise ValueError("chain_hist_begin: pairs must be (P, 2) integers, got %s %s" % (pr.dtype, pr.shape))
        pr = np.ascontiguousarray(pr, dtype=np.int32)
        if edges2 is None:
            if len(pr):
                raise ValueError("chain_hist_begin: pairs need edges2")
            e2 = np.zeros((self.p, 3))
            e2[:, 1:] = (1.0, 2.0)
        else:
            e2 = np.ascontiguousarray(np.asarray(edges2, dtype=np.float64))
        if e2.ndim != 2 or e2.shape[0] != self.p:
            raise ValueError("chain_hist_begin: edges2 must have shape (%d, bins2d + 1), got %s" % (self.p, e2.shape))
        d = ChainHistDesc()
        d.struct_bytes = C.sizeof(ChainHistDesc)
        d.bins, d.bins2d, d.n_pairs = e1.shape[1] - 1, e2.shape[1] - 1, len(pr)
        d.edges1, d.edges2, d.pairs = e1.ctypes.data, e2.ctypes.data, pr.ctypes.data if len(pr) else None
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_chain_hist_begin(self._h, C.byref(d), self._stream()))
        self._chain_hist_shape = (d.bins, d.bins2d, len(pr))

    def chain_hist_add(self, trace):
        """Count the draws of ``trace``, (kept, p, J) or one state (p, J), engine dtype (cesx_chain_hist_add): the argument
        of ``chain_summary_add``.  Nothing is copied: the kernels read ``trace`` on the current stream."""
        shape = tuple(trace.shape)
        if (trace.dtype != self.torch_dtype or not trace.is_cuda or not trace.is_contiguous()
                or shape[-2:] != (self.p, self.J) or len(shape) not in (2, 3)):
            raise ValueError("chain_hist_add: trace must be a contiguous %s tensor of shape (kept, %d, %d) or (%d, %d)"
                             % (self.torch_dtype, self.p, self.J, self.p, self.J))
        kept = shape[0] if len(shape) == 3 else 1
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_chain_hist_add(self._h, trace.data_ptr(), kept, self._stream()))
        self._keep_chain_hist = trace

    def chain_hist_read(self):
        """The run's counts so far as host int64 arrays (cesx_chain_hist_read): ``hist1d`` (p, bins), ``below`` and ``above``
        (p,), ``hist2d`` (P, bins2d, bins2d) -- row the bin of a pair's first parameter, column that of its second -- and
        ``outside2d`` (P,).  Synchronises; the run goes on."""
        if self._chain_hist_shape is None:
            raise CesxError(ESTATE, "chain_hist_read: chain_hist_begin has not been called")
        B, B2, P = self._chain_hist_shape
        h1, o1 = np.zeros((self.p, B), dtype=np.uint64), np.zeros((self.p, 2), dtype=np.uint64)
        h2, o2 = np.zeros((P, B2, B2), dtype=np.uint64), np.zeros(P, dtype=np.uint64)
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_chain_hist_read(self._h, h1.ctypes.data, o1.ctypes.data, h2.ctypes.data if P else None,
                                                      o2.ctypes.data if P else None, self._stream()))
        self._keep_chain_hist = None
        return dict(hist1d=h1.astype(np.int64), below=o1[:, 0].astype(np.int64), above=o1[:, 1].astype(np.int64),
                    hist2d=h2.astype(np.int64), outside2d=o2.astype(np.int64))

    # -- streaming lagged sums of the chains' draws (include/cesx.h, cesx_chain_acf_*) --
    def chain_acf_begin(self, n_draws, lags, chains):
        """Clear the stage for a run of ``n_draws`` draws per chain, lags 0 .. ``lags`` and the first ``chains`` chains
        (cesx_chain_acf_begin).  ValueError for a limit of include/cesx.h; the run in hand then goes on."""
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_chain_acf_begin(self._h, int(n_draws), int(lags), int(chains), self._stream()))
        self._chain_acf_shape = (int(lags), int(chains))

    def chain_acf_add(self, trace):
        """Add the draws of ``trace``, (kept, p, J) or one state (p, J), engine dtype, in order (cesx_chain_acf_add): the
        argument of ``chain_summary_add``.  Fewer than 64 draws are copied into the stage's own memory; more are read in place."""
        shape = tuple(trace.shape)
        if (trace.dtype != self.torch_dtype or not trace.is_cuda or not trace.is_contiguous()
                or shape[-2:] != (self.p, self.J) or len(shape) not in (2, 3)):
            raise ValueError("chain_acf_add: trace must be a contiguous %s tensor of shape (kept, %d, %d) or (%d, %d)"
                             % (self.torch_dtype, self.p, self.J, self.p, self.J))
        kept = shape[0] if len(shape) == 3 else 1
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_chain_acf_add(self._h, trace.data_ptr(), kept, self._stream()))
        self._keep_chain_acf = trace

    def chain_acf_read(self, chains=False):
        """The run's raw sums as host fp64 arrays (cesx_chain_acf_read): ``gsum`` (p, lags + 1), ``msum`` (p,), ``m2sum`` (p,);
        with ``chains`` also every chain's ``chain_gamma`` (lags + 1, p, C) and ``chain_mean`` (p, C).  Synchronises."""
        if self._chain_acf_shape is None:
            raise CesxError(ESTATE, "chain_acf_read: chain_acf_begin has not been called")
        L, Cn = self._chain_acf_shape
        p = self.p
        out = dict(gsum=np.empty((p, L + 1)), msum=np.empty(p), m2sum=np.empty(p))
        if chains:
            out.update(chain_gamma=np.empty((L + 1, p, Cn)), chain_mean=np.empty((p, Cn)))
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_chain_acf_read(self._h, out["gsum"].ctypes.data, out["msum"].ctypes.data, out["m2sum"].ctypes.data,
                                                     out["chain_gamma"].ctypes.data if chains else None,
                                                     out["chain_mean"].ctypes.data if chains else None, self._stream()))
        self._keep_chain_acf = None
        return out

    def profile_enable(self, on=True):
        """on: False / True, 2 = bind only the events cesx_profile_gap needs, 3 / 4 = the update / the moments
        launches alone."""
        mode = int(on) if (on is not True and on is not False and on in (2, 3, 4)) else int(bool(on))
        self._check(self.lib.cesx_profile_enable(self._h, mode))

    def profile_read(self, which):
        """(total ms, launches) of kernel 0 = Gram (K1) or 1 = update (K3) since the last read."""
        ms, cnt = C.c_double(), C.c_int()
        self._check(self.lib.cesx_profile_read(self._h, int(which), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def profile_gap(self):
        """ms from the end of the last profiled Gram launch to the start of the last profiled update launch
        (cesx_profile_gap; call before profile_read); None when nothing was profiled."""
        ms = C.c_double()
        self._check(self.lib.cesx_profile_gap(self._h, C.byref(ms)))
        return ms.value if ms.value >= 0 else None

    def profile_clock(self):
        """Shader clock (GHz) of the last profiled update launch (cesx_profile_clock)."""
        ghz = C.c_double()
        self._check(self.lib.cesx_profile_clock(self._h, C.byref(ghz)))
        return ghz.value

    def calibrate_mfma(self, target_ms=5.0):
        """(TFLOP/s, GHz) of a bare MFMA loop of the engine dtype on this device (cesx_calibrate_mfma)."""
        tf, ghz = C.c_double(), C.c_double()
        with torch.cuda.device(self.device):
            self._check(self.lib.cesx_calibrate_mfma(self._h, float(target_ms), C.byref(tf), C.byref(ghz), self._stream()))
        return tf.value, ghz.value

    def debug_dense(self):
        p, n = self.p, self.n_obs
        out = dict(ubar=np.empty(p), gbar=np.empty(n), C=np.empty((p, p)), L=np.empty((p, p)),
                   K=np.empty((p, n)), M=np.empty((p, p)))
        self._check(self.lib.cesx_debug_dense(self._h, _dptr(out["ubar"]), _dptr(out["gbar"]), _dptr(out["C"]),
                                              _dptr(out["L"]), _dptr(out["K"]), _dptr(out["M"])))
        return out
