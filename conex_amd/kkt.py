"""ctypes binding of the cxk_* C-ABI (include/conex_kkt_hip.h).

Mirrors conex::Program / SupernodalKKTSolver method names (cone_program.h:99-233,
kkt_solver.h:16-65) so parity tests read like the reference's own tests.
"""
import ctypes as C
import os

import numpy as np

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libconex.so")
_LIB = None

c_int_p = C.POINTER(C.c_int)
c_long_p = C.POINTER(C.c_long)
c_double_p = C.POINTER(C.c_double)


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def _ip(a):
    return a.ctypes.data_as(c_int_p)


def _lp(a):
    return a.ctypes.data_as(c_long_p)


_SIGNATURES = {
    "cxk_create": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "cxk_destroy": (None, [C.c_void_p]),
    "cxk_last_error": (C.c_char_p, [C.c_void_p]),
    "cxk_add_lmi": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p, c_int_p]),
    "cxk_add_lmi_factored": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_int_p, c_double_p, c_double_p, c_double_p, c_int_p]),
    "cxk_count_factored_lmi": (C.c_int, [C.c_void_p]),
    "cxk_add_hermitian_factored": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_int_p, c_double_p, c_double_p, c_double_p,
                                             c_int_p]),
    "cxk_add_linear": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p, c_int_p]),
    "cxk_add_soc": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p, c_int_p]),
    "cxk_add_quadratic": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_int_p]),
    "cxk_add_equality": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p, c_int_p]),
    "cxk_factor_regularized": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "cxk_add_hermitian": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_double_p, c_double_p,
                                    c_int_p]),
    "cxk_add_static": (C.c_int, [C.c_void_p, C.c_int, c_double_p, c_int_p]),
    "cxk_num_constraints": (C.c_int, [C.c_void_p]),
    "cxk_set_shard": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "cxk_finalize": (C.c_int, [C.c_void_p]),
    "cxk_system_size": (C.c_int, [C.c_void_p]),
    "cxk_get_order": (C.c_int, [C.c_void_p, c_int_p]),
    "cxk_get_permutation": (C.c_int, [C.c_void_p, c_int_p, c_int_p]),
    "cxk_get_list": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_int_p]),
    "cxk_get_supernode_sizes": (C.c_int, [C.c_void_p, c_int_p]),
    "cxk_slab_size": (C.c_long, [C.c_void_p]),
    "cxk_get_block_offsets": (C.c_int, [C.c_void_p, c_long_p, c_long_p]),
    "cxk_get_ss_index": (C.c_int, [C.c_void_p, C.c_int, c_long_p]),
    "cxk_num_levels": (C.c_int, [C.c_void_p]),
    "cxk_set_identity": (C.c_int, [C.c_void_p]),
    "cxk_dual_size": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_get_W": (C.c_int, [C.c_void_p, C.c_int, c_double_p]),
    "cxk_set_W": (C.c_int, [C.c_void_p, C.c_int, c_double_p]),
    "cxk_assemble": (C.c_int, [C.c_void_p]),
    "cxk_factor": (C.c_int, [C.c_void_p, c_int_p]),
    "cxk_set_cost": (C.c_int, [C.c_void_p, c_double_p]),
    "cxk_newton_direction": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "cxk_solve_rhs": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "cxk_step_scalars": (C.c_int, [C.c_void_p, c_double_p]),
    "cxk_kkt_solve_async": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "cxk_sync": (C.c_int, [C.c_void_p, c_int_p]),
    "cxk_solve_inplace": (C.c_int, [C.c_void_p, c_double_p]),
    "cxk_get_y": (C.c_int, [C.c_void_p, c_double_p]),
    "cxk_set_y": (C.c_int, [C.c_void_p, c_double_p]),
    "cxk_prepare_step": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, c_double_p]),
    "cxk_take_step": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double]),
    "cxk_prepare_take_step": (C.c_int, [C.c_void_p, C.c_double, C.c_double, c_double_p, C.POINTER(C.c_int)]),
    "cxk_weighted_slack_eigenvalues": (C.c_int, [C.c_void_p, C.c_double, c_double_p]),
    "cxk_get_slab": (C.c_int, [C.c_void_p, c_double_p]),
    "cxk_set_slab": (C.c_int, [C.c_void_p, c_double_p]),
    "cxk_get_constraint_schur": (C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p,
                                           c_double_p, c_double_p]),
    "cxk_get_residuals": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    "cxk_exchange_buffer": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), c_long_p]),
    "cxk_exchange_download": (C.c_int, [C.c_void_p, c_double_p]),
    "cxk_exchange_upload": (C.c_int, [C.c_void_p, c_double_p]),
    "cxk_kkt_local_async": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "cxk_kkt_finish_async": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "cxk_owns_constraint": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_get_valid_variables": (C.c_int, [C.c_void_p, C.POINTER(C.c_ubyte)]),
    "cxk_shard_info": (C.c_int, [C.c_void_p, c_int_p, c_int_p, c_long_p]),
    "cxk_assemble_local": (C.c_int, [C.c_void_p]),
    "cxk_finish_assemble": (C.c_int, [C.c_void_p]),
    "cxk_assembly_work": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "cxk_count_sparse_lmi": (C.c_int, [C.c_void_p]),
    "cxk_count_lmi_kernel": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_lmi_kernels": (C.c_int, [C.c_void_p, C.c_int, c_int_p]),
    "cxk_lmi_kernel_name": (C.c_char_p, [C.c_int]),
    "cxk_lmi_kernel_count": (C.c_int, []),
    "cxk_get_step_info": (C.c_int, [C.c_void_p, c_double_p]),
    "cxk_line_search": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, c_double_p]),
    "cxk_fused_assembly": (C.c_int, [C.c_void_p]),
    "cxk_fused_tree": (C.c_int, [C.c_void_p]),
    "cxk_comm_init_rccl_solo": (C.c_int, [C.c_void_p]),
    "cxk_set_reference_identity": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_set_solver_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_phase_timers": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_phase_mark": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_phase_read": (C.c_int, [C.c_void_p, c_double_p, C.c_int]),
    "cxk_comm_unique_id": (C.c_int, [C.c_void_p]),
    "cxk_comm_init_rccl": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "cxk_comm_set_allreduce": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cxk_comm_selftest": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_comm_count": (C.c_int, [C.c_void_p]),
    "cxk_dense_top_columns": (C.c_int, [C.c_void_p]),
    "cxk_factor_async": (C.c_int, [C.c_void_p]),
    "cxk_factor_solve_async": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "cxk_factor_direction_async": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "cxk_factor_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "cxk_step_scalars_async": (C.c_int, [C.c_void_p]),
    "cxk_device_mu_supported": (C.c_int, [C.c_void_p]),
    "cxk_triple_supported": (C.c_int, [C.c_void_p]),
    "cxk_factor_solve_triple_async": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "cxk_select_mu_async": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                                      C.c_double]),
    "cxk_newton_direction_device_mu": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "cxk_prepare_take_step_device_mu": (C.c_int, [C.c_void_p, C.c_double, C.c_double, c_double_p,
                                                  C.POINTER(C.c_int), c_double_p]),
    "cxk_kernel_time": (C.c_int, [C.c_void_p, C.c_int, c_double_p]),
    "cxk_enable_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_kernel_clock": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p]),
    "cxk_set_chain_segments": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_chain_segments": (C.c_int, [C.c_void_p]),
    "cxk_set_streamed_cones": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_count_streamed_cones": (C.c_int, [C.c_void_p]),
    "cxk_set_streamed_quadratic": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_count_streamed_quadratic": (C.c_int, [C.c_void_p]),
    "cxk_add_quadratic_structured": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_int_p, c_int_p, c_double_p, C.c_int, c_double_p,
                                               c_double_p, c_double_p, c_double_p, c_int_p]),
    "cxk_count_structured_quadratic": (C.c_int, [C.c_void_p]),
    "cxk_add_quadratic_csr": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p, c_int_p, c_int_p, c_double_p, C.c_int, c_double_p,
                                        c_double_p, c_int_p, c_int_p, c_double_p, c_double_p, c_int_p]),
    "cxk_count_sparse_quadratic": (C.c_int, [C.c_void_p]),
    "cxk_set_tiled_linear": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_set_sparse_linear": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_count_sparse_linear": (C.c_int, [C.c_void_p]),
    "cxk_add_linear_csr": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_int_p, c_int_p, c_double_p, c_double_p, c_int_p]),
    "cxk_set_sparse_soc": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_count_sparse_soc": (C.c_int, [C.c_void_p]),
    "cxk_sparse_soc_setup_ms": (C.c_double, [C.c_void_p]),
    "cxk_set_wide_spectrum": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_count_wide_spectrum": (C.c_int, [C.c_void_p]),
    "cxk_add_soc_csr": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_int_p, c_int_p, c_double_p, c_double_p, c_int_p]),
    "cxk_add_lmi_coo": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, c_double_p, c_int_p]),
    "cxk_set_sparse_affine": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_count_sparse_affine": (C.c_int, [C.c_void_p]),
    "cxk_add_hermitian_coo": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, c_double_p, c_int_p]),
    "cxk_set_sparse_fold": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_count_sparse_fold": (C.c_int, [C.c_void_p]),
    "cxk_count_tiled_linear": (C.c_int, [C.c_void_p]),
    "cxk_fused_tree_timed_out": (C.c_int, [C.c_void_p]),
    "cxk_debug_force_fused_timeout": (C.c_int, [C.c_void_p]),
    "cxk_debug_fused_timeout_at": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "cxk_set_iterative_refinement": (C.c_int, [C.c_void_p, C.c_int]),
    "cxk_solve_block": (C.c_int, [C.c_void_p, c_double_p, C.c_int, C.c_int]),
    "cxk_solve_block_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "cxk_solve_block_chunk_width": (C.c_int, []),
}


def load_library():
    """Load libconex.so; raises (loudly) when the HIP library has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP library first (python __graft_entry__.py or "
            "make -C conex_amd/csrc). There is no CPU fallback for the KKT path.")
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError if an ABI symbol is missing
        fn.restype = res
        fn.argtypes = args
    _LIB = L
    return L


# stages of cxk_lmi_kernels, in the order of its output (CXK_LMI_STAGE_*)
LMI_STAGES = ("schur", "prepare", "query", "take", "affine")


def lmi_kernel_names():
    """Every kernel instance name cxk_lmi_kernels can report, in code order."""
    L = load_library()
    return [L.cxk_lmi_kernel_name(c).decode() for c in range(L.cxk_lmi_kernel_count())]


def _colmajor(a):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 2:
        return np.ascontiguousarray(a.T).ravel()
    if a.ndim == 3:
        return np.ascontiguousarray(np.transpose(a, (0, 2, 1))).ravel()
    return np.ascontiguousarray(a).ravel()


class KktError(RuntimeError):
    pass


def csr_triple(S, rows, name="S"):
    """(indptr, indices, data) as contiguous int32 / int32 / float64 arrays of a matrix of `rows` rows held in CSR: S is a
    triple or any object with the attributes indptr, indices and data (a scipy CSR matrix; scipy itself is not needed)."""
    if all(hasattr(S, a) for a in ("indptr", "indices", "data")):
        S = (S.indptr, S.indices, S.data)
    try:
        indptr, indices, data = S
    except (TypeError, ValueError):
        raise ValueError("%s is %s(indptr, indices, data) or an object with those attributes"
                         % (name, "None, " if name == "S" else "")) from None
    ip64, ix64 = np.asarray(indptr).ravel(), np.asarray(indices).ravel()
    if ip64.dtype.kind not in "iu" or (len(ix64) and ix64.dtype.kind not in "iu"):
        raise ValueError("%s: indptr and indices are integers" % name)
    if len(ip64) and (ip64.max() > 2 ** 31 - 1 or ip64.min() < -2 ** 31):
        raise ValueError("%s: indptr beyond the int range" % name)
    if len(ix64) and (ix64.max() > 2 ** 31 - 1 or ix64.min() < -2 ** 31):
        raise ValueError("%s: indices beyond the int range" % name)
    rp = np.ascontiguousarray(ip64, dtype=np.int32)
    cl = np.ascontiguousarray(ix64, dtype=np.int32)
    vl = np.ascontiguousarray(np.asarray(data, dtype=np.float64).ravel())
    if len(rp) != rows + 1 or len(cl) != len(vl) or (len(rp) and rp[-1] > len(vl)):
        raise ValueError("%s: indptr has %s + 1 entries and points into indices / data of equal length"
                         % (name, "n" if name == "S" else "rows"))
    return rp, cl, vl


def structured_q_parts(S, n):
    """csr_triple of the sparse part of a structured Q of order n, or (None, None, None) where S is None."""
    if S is None:
        return None, None, None
    return csr_triple(S, n)


def quadratic_q_forms(Q, n, who):
    """(dense, (rp, cl, vl), rank, F, sigma) of a quadratic cone's Q as add_quadratic_csr and
    Conex.AddSparseQuadraticConstraint take it: None (the identity), an (n, n) array, or the parts -- a dict with any of
    the keys S, F, sigma, or a tuple (S, F, sigma) -- in the forms add_quadratic_structured takes.  Column-major
    float64 copies; what is absent is None."""
    none3 = (None, None, None)
    if Q is None:
        return None, none3, 0, None, None
    if isinstance(Q, dict):
        S, F, sigma = Q.get("S"), Q.get("F"), Q.get("sigma")
    elif isinstance(Q, tuple) and len(Q) == 3:
        S, F, sigma = Q
    else:
        Qa = np.asarray(Q, dtype=np.float64)
        if Qa.shape != (n, n):
            raise ValueError("%s: Q is None, (n, n), or the parts (S, F, sigma)" % who)
        return _colmajor(Qa), none3, 0, None, None
    rank, f, sg = 0, None, None
    if F is not None:
        F = np.asarray(F, dtype=np.float64)
        if F.ndim != 2 or F.shape[0] != n:
            raise ValueError("%s: F is (n, r)" % who)
        rank = F.shape[1]
        f = _colmajor(F)
    if sigma is not None:
        sg = np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).ravel())
        if len(sg) != rank:
            raise ValueError("%s: sigma has one entry per column of F" % who)
    if S is None and rank == 0:
        raise ValueError("%s: neither a sparse part nor factors (for the identity pass Q = None)" % who)
    return None, structured_q_parts(S, n), rank, f, sg


class KktContext:
    """Device-resident cone program (one HIP device, one stream)."""

    def __init__(self, num_vars, device=0, stream=None):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.cxk_create(num_vars, device, C.c_void_p(stream) if stream else None,
                               C.byref(h))
        if rc != 0:
            raise KktError(f"cxk_create failed for device {device} (no usable HIP device?)")
        self.h = h
        self.stream = stream
        self.num_vars = num_vars
        self.cons = []

    def close(self):
        if getattr(self, "h", None):
            self.L.cxk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise KktError(f"{what}: {self.L.cxk_last_error(self.h).decode()}")

    @staticmethod
    def _vars(v):
        if v is None:
            return None, None
        a = np.ascontiguousarray(v, dtype=np.int32)
        return a, _ip(a)

    # ---- construction
    def add_lmi(self, A, Cm, vars_=None):
        A = np.asarray(A, dtype=np.float64)
        m, n = A.shape[0], A.shape[1]
        a, c = _colmajor(A), _colmajor(np.asarray(Cm, dtype=np.float64))
        keep, vp = self._vars(vars_)
        r = self.L.cxk_add_lmi(self.h, n, m, _dp(a), _dp(c), vp)
        if r >= 0:
            self.cons.append(("lmi", n, m))
        return r

    def add_lmi_factored(self, F, rank_ptr, sigma, Cm, vars_=None):
        """The constraint of add_lmi with A_i = sum_k sigma[k] F[:, k] F[:, k]', k in rank_ptr[i]:rank_ptr[i + 1]: F is
        n x R, rank_ptr has m + 1 entries, sigma R signs or weights (None: all +1).  The A_i are never formed."""
        Cm = np.asarray(Cm, dtype=np.float64)
        n = Cm.shape[0]
        rp = np.ascontiguousarray(rank_ptr, dtype=np.int32)
        F = np.asarray(F, dtype=np.float64).reshape(n, -1)
        sg = None if sigma is None else np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).ravel())
        if len(rp) < 1 or (len(rp) and rp[-1] != F.shape[1]) or (sg is not None and len(sg) != F.shape[1]):
            raise ValueError("add_lmi_factored: rank_ptr ends at the number of columns of F, which sigma has one entry for")
        f, c = _colmajor(F), _colmajor(Cm)
        keep, vp = self._vars(vars_)
        m = len(rp) - 1
        r = self.L.cxk_add_lmi_factored(self.h, n, m, _ip(rp), _dp(f), None if sg is None else _dp(sg), _dp(c), vp)
        if r >= 0:
            self.cons.append(("lmi", n, m))
        return r

    def add_lmi_coo(self, n, ptr, row, col, val, vars_=None):
        """The constraint of add_lmi, of order n, by the entries of the lower triangles: list i, row / col / val
        [ptr[i]:ptr[i + 1]] with row >= col, holds A_i and the last list holds C; ptr has m + 2 entries, m = len(vars_)
        or the context's variables.  Entries of a list in any order; explicit zeros are dropped.  The matrices are never
        formed, and the constraint takes the sparse route only."""
        pt = np.ascontiguousarray(ptr, dtype=np.int32)
        rw = np.ascontiguousarray(row, dtype=np.int32)
        cl = np.ascontiguousarray(col, dtype=np.int32)
        vl = np.ascontiguousarray(val, dtype=np.float64)
        keep, vp = self._vars(vars_)
        m = self.num_vars if vars_ is None else len(keep)
        if len(pt) != m + 2 or not (len(rw) == len(cl) == len(vl)) or pt[-1] > len(vl):
            raise ValueError("add_lmi_coo: ptr has m + 2 entries and points into row / col / val of equal length")
        r = self.L.cxk_add_lmi_coo(self.h, int(n), m, _ip(pt), _ip(rw), _ip(cl), _dp(vl), vp)
        if r >= 0:
            self.cons.append(("lmi", int(n), m))
        return r

    def add_linear(self, A, c, vars_=None):
        A = np.asarray(A, dtype=np.float64)
        rows, m = A.shape
        a = _colmajor(A)
        cc = np.ascontiguousarray(np.asarray(c, dtype=np.float64).ravel())
        keep, vp = self._vars(vars_)
        r = self.L.cxk_add_linear(self.h, rows, m, _dp(a), _dp(cc), vp)
        if r >= 0:
            self.cons.append(("linear", rows, m))
        return r

    def add_linear_csr(self, rowptr, col, val, c, vars_=None):
        """The constraint of add_linear by its nonzeros: row r holds col / val [rowptr[r]:rowptr[r + 1]], columns in any
        order.  The number of variables is len(vars_), or the context's.  Such a block takes the sparse route only."""
        rp = np.ascontiguousarray(rowptr, dtype=np.int32)
        cl = np.ascontiguousarray(col, dtype=np.int32)
        vl = np.ascontiguousarray(val, dtype=np.float64)
        cc = np.ascontiguousarray(np.asarray(c, dtype=np.float64).ravel())
        rows = len(cc)
        if len(rp) != rows + 1 or len(cl) != len(vl) or (len(rp) and rp[-1] > len(cl)):
            raise ValueError("add_linear_csr: rowptr has len(c) + 1 entries and points into col / val of equal length")
        keep, vp = self._vars(vars_)
        m = self.num_vars if vars_ is None else len(keep)
        r = self.L.cxk_add_linear_csr(self.h, rows, m, _ip(rp), _ip(cl), _dp(vl), _dp(cc), vp)
        if r >= 0:
            self.cons.append(("linear", rows, m))
        return r

    def add_soc_csr(self, rowptr, col, val, c, vars_=None):
        """The constraint of add_soc by the nonzeros of its (n + 1) x m matrix: row r holds col / val
        [rowptr[r]:rowptr[r + 1]], columns in any order; n + 1 = len(c).  The number of variables is len(vars_), or the
        context's.  Such a cone takes the sparse route only."""
        rp = np.ascontiguousarray(rowptr, dtype=np.int32)
        cl = np.ascontiguousarray(col, dtype=np.int32)
        vl = np.ascontiguousarray(val, dtype=np.float64)
        cc = np.ascontiguousarray(np.asarray(c, dtype=np.float64).ravel())
        rows = len(cc)
        if len(rp) != rows + 1 or len(cl) != len(vl) or (len(rp) and rp[-1] > len(cl)):
            raise ValueError("add_soc_csr: rowptr has len(c) + 1 entries and points into col / val of equal length")
        keep, vp = self._vars(vars_)
        m = self.num_vars if vars_ is None else len(keep)
        r = self.L.cxk_add_soc_csr(self.h, rows - 1, m, _ip(rp), _ip(cl), _dp(vl), _dp(cc), vp)
        if r >= 0:
            self.cons.append(("soc", rows - 1, m))
        return r

    def add_hermitian(self, A, Cm, vars_=None):
        """Hermitian PSD over R / C / H / O: A (m, d, n, n) real planes, Cm (d, n, n); d in {1, 2, 4, 8}
        (octonions, d = 8: order at most 3)."""
        A = np.asarray(A, dtype=np.float64)
        m, d, n = A.shape[0], A.shape[1], A.shape[2]
        a = np.ascontiguousarray(np.swapaxes(A, -1, -2)).ravel()
        c = np.ascontiguousarray(np.swapaxes(np.asarray(Cm, dtype=np.float64), -1, -2)).ravel()
        keep, vp = self._vars(vars_)
        r = self.L.cxk_add_hermitian(self.h, n, d, m, _dp(a), _dp(c), vp)
        if r >= 0:
            self.cons.append(("herm", n, m, d))
        return r

    def add_hermitian_coo(self, n, d, ptr, row, col, val, vars_=None):
        """The constraint of add_hermitian, of order n over R / C / H (d = 1, 2, 4), by the entries of the lower
        triangles: the lists as for add_lmi_coo; val is (nnz, d) real planes, or a complex array for d = 2.  The upper
        triangle is the conjugate.  Neither the matrices nor their real representations are formed, and the constraint
        takes the sparse route only."""
        pt = np.ascontiguousarray(ptr, dtype=np.int32)
        rw = np.ascontiguousarray(row, dtype=np.int32)
        cl = np.ascontiguousarray(col, dtype=np.int32)
        vl = np.asarray(val)
        if np.iscomplexobj(vl):
            if int(d) != 2 or vl.ndim != 1:
                raise ValueError("add_hermitian_coo: a complex val is one number per entry, for d = 2")
            vl = np.stack([vl.real, vl.imag], axis=1)
        vl = np.ascontiguousarray(vl, dtype=np.float64)
        if vl.ndim == 1 and int(d) == 1:
            vl = vl.reshape(-1, 1)
        keep, vp = self._vars(vars_)
        m = self.num_vars if vars_ is None else len(keep)
        if vl.ndim != 2 or vl.shape[1] != int(d):
            raise ValueError("add_hermitian_coo: val is (nnz, d) planes")
        if len(pt) != m + 2 or not (len(rw) == len(cl) == len(vl)) or pt[-1] > len(vl):
            raise ValueError("add_hermitian_coo: ptr has m + 2 entries and points into row / col / val of equal length")
        r = self.L.cxk_add_hermitian_coo(self.h, int(n), int(d), m, _ip(pt), _ip(rw), _ip(cl), _dp(vl), vp)
        if r >= 0:
            self.cons.append(("herm", int(n), m, int(d)))
        return r

    def add_hermitian_factored(self, F, rank_ptr, sigma, Cm, vars_=None):
        """The constraint of add_hermitian with A_i = sum_k sigma[k] f_k f_k^*, k in rank_ptr[i]:rank_ptr[i + 1], f_k the
        hyper-complex columns of F: F is (d, n, R) real planes, d in {1, 2, 4}, Cm (d, n, n), rank_ptr has m + 1 entries,
        sigma R signs or weights (None: all +1).  Neither the A_i nor their real representations are formed."""
        Cm = np.asarray(Cm, dtype=np.float64)
        F = np.asarray(F, dtype=np.float64)
        if Cm.ndim != 3 or Cm.shape[1] != Cm.shape[2] or F.ndim != 3 or F.shape[:2] != Cm.shape[:2]:
            raise ValueError("add_hermitian_factored: F is (d, n, R) planes and Cm (d, n, n) planes of the same d and n")
        d, n, R = F.shape
        rp = np.ascontiguousarray(rank_ptr, dtype=np.int32)
        sg = None if sigma is None else np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).ravel())
        if len(rp) < 1 or rp[-1] != R or (sg is not None and len(sg) != R):
            raise ValueError("add_hermitian_factored: rank_ptr ends at the number of columns of F, which sigma has one entry for")
        f = np.ascontiguousarray(np.swapaxes(F, -1, -2)).ravel()
        c = np.ascontiguousarray(np.swapaxes(Cm, -1, -2)).ravel()
        keep, vp = self._vars(vars_)
        m = len(rp) - 1
        r = self.L.cxk_add_hermitian_factored(self.h, n, d, m, _ip(rp), _dp(f), None if sg is None else _dp(sg), _dp(c), vp)
        if r >= 0:
            self.cons.append(("herm", n, m, d))
        return r

    def add_equality(self, A, b, vars_=None):
        """A y[vars] = b; appends A.shape[0] multipliers and switches the solver to LDLT."""
        A = np.asarray(A, dtype=np.float64)
        rows, m = A.shape
        a = _colmajor(A)
        bb = np.ascontiguousarray(np.asarray(b, dtype=np.float64).ravel())
        keep, vp = self._vars(vars_)
        r = self.L.cxk_add_equality(self.h, rows, m, _dp(a), _dp(bb), vp)
        if r >= 0:
            self.cons.append(("eq", rows, m + rows))
        return r

    def factor_regularized(self):
        f = C.c_int(0)
        self._check(self.L.cxk_factor_regularized(self.h, C.byref(f)), "cxk_factor_regularized")
        return f.value

    def add_soc(self, A, c, vars_=None):
        A = np.asarray(A, dtype=np.float64)
        n1, m = A.shape
        a = _colmajor(A)
        cc = np.ascontiguousarray(np.asarray(c, dtype=np.float64).ravel())
        keep, vp = self._vars(vars_)
        r = self.L.cxk_add_soc(self.h, n1 - 1, m, _dp(a), _dp(cc), vp)
        if r >= 0:
            self.cons.append(("soc", n1 - 1, m))
        return r

    def add_quadratic(self, Q, A, c, vars_=None):
        """QuadraticConstraint(Q, A, c): Q (n, n) or None (identity), A (n + 1, m), c (n + 1,)."""
        A = np.asarray(A, dtype=np.float64)
        n1, m = A.shape
        a = _colmajor(A)
        cc = np.ascontiguousarray(np.asarray(c, dtype=np.float64).ravel())
        q = None if Q is None else _colmajor(np.asarray(Q, dtype=np.float64))
        keep, vp = self._vars(vars_)
        r = self.L.cxk_add_quadratic(self.h, n1 - 1, m, None if q is None else _dp(q), _dp(a), _dp(cc), vp)
        if r >= 0:
            self.cons.append(("quad", n1 - 1, m))
        return r

    def add_quadratic_structured(self, S, F, sigma, A, c, vars_=None):
        """The cone of add_quadratic with Q = S + F diag(sigma) F' given by its parts and never formed.  S: None, a triple
        (indptr, indices, data) or any object with those three attributes (a scipy CSR matrix), n x n with both
        triangles stored; F: None or (n, r); sigma: None (all +1) or (r,).  Not both S and F None."""
        A = np.asarray(A, dtype=np.float64)
        n1, m = A.shape
        a = _colmajor(A)
        cc = np.ascontiguousarray(np.asarray(c, dtype=np.float64).ravel())
        rp, cl, vl = structured_q_parts(S, n1 - 1)
        f = sg = None
        rank = 0
        if F is not None:
            F = np.asarray(F, dtype=np.float64)
            if F.ndim != 2 or F.shape[0] != n1 - 1:
                raise ValueError("add_quadratic_structured: F is (n, r)")
            rank = F.shape[1]
            f = _colmajor(F)
        if sigma is not None:
            sg = np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).ravel())
            if len(sg) != rank:
                raise ValueError("add_quadratic_structured: sigma has one entry per column of F")
        keep, vp = self._vars(vars_)
        r = self.L.cxk_add_quadratic_structured(
            self.h, n1 - 1, m, None if rp is None else _ip(rp), None if rp is None else _ip(cl),
            None if rp is None else _dp(vl), rank, None if f is None or rank == 0 else _dp(f), None if sg is None else _dp(sg),
            _dp(a), _dp(cc), vp)
        if r < 0:  # refused by name (the context stays usable)
            raise KktError(self.L.cxk_last_error(self.h).decode() or "cxk_add_quadratic_structured: invalid arguments")
        self.cons.append(("quad", n1 - 1, m))
        return r

    def count_structured_quadratic(self):
        """Constraints this context owns that were added by add_quadratic_structured."""
        return self.L.cxk_count_structured_quadratic(self.h)

    def add_quadratic_csr(self, Q, A, c, vars_=None):
        """The cone of add_quadratic / add_quadratic_structured with its (n + 1) x m matrix A given by its nonzeros and
        never formed.  A: a triple (indptr, indices, data) or any object with those three attributes (a scipy CSR
        matrix), row 0 is A0; columns in any order within a row, explicit zeros dropped; as many columns as vars_ has
        entries (every variable without vars_).  Q: None (the identity), an (n, n) array, or the parts as a dict(S=, F=, sigma=) or a tuple (S, F, sigma), each as add_quadratic_structured
        takes it."""
        cc = np.ascontiguousarray(np.asarray(c, dtype=np.float64).ravel())
        n = len(cc) - 1
        rp, cl, vl = csr_triple(A, n + 1, "A")
        keep, vp = self._vars(vars_)
        m = self.num_vars if vars_ is None else len(keep)
        dense, (qp, qc, qv), rank, f, sg = quadratic_q_forms(Q, n, "add_quadratic_csr")
        r = self.L.cxk_add_quadratic_csr(
            self.h, n, m, None if dense is None else _dp(dense), None if qp is None else _ip(qp), None if qp is None else _ip(qc),
            None if qp is None else _dp(qv), rank, None if f is None or rank == 0 else _dp(f), None if sg is None else _dp(sg),
            _ip(rp), _ip(cl), _dp(vl), _dp(cc), vp)
        if r < 0:  # refused by name (the context stays usable)
            raise KktError(self.L.cxk_last_error(self.h).decode() or "cxk_add_quadratic_csr: invalid arguments")
        self.cons.append(("quad", n, m))
        return r

    def count_sparse_quadratic(self):
        """Constraints this context owns that were added by add_quadratic_csr."""
        return self.L.cxk_count_sparse_quadratic(self.h)

    def add_static(self, G, vars_):
        G = np.asarray(G, dtype=np.float64)
        m = G.shape[0]
        g = _colmajor(G)
        keep, vp = self._vars(vars_)
        r = self.L.cxk_add_static(self.h, m, _dp(g), vp)
        if r >= 0:
            self.cons.append(("static", 0, m))
        return r

    def set_shard(self, rank, world):
        self._check(self.L.cxk_set_shard(self.h, rank, world), "cxk_set_shard")

    def initialize(self):
        self._check(self.L.cxk_finalize(self.h), "cxk_finalize")
        return 1

    # ---- symbolic
    @property
    def K(self):
        return self.L.cxk_num_constraints(self.h)

    @property
    def N(self):
        return self.L.cxk_system_size(self.h)

    @property
    def span(self):
        """Entries of a vector in the original variable order (get_y, set_y, solve_inplace, residuals,
        valid_variables): one per variable of the context and per multiplier (V of include/conex_kkt_hip.h).  Equal to
        N when every variable occurs in a constraint; the library indexes such vectors by variable, so a context that
        leaves variables out has span > N."""
        return max(self.N, self.num_vars + sum(c[1] for c in self.cons if c[0] == "eq"))

    def order(self):
        o = np.zeros(self.K, dtype=np.int32)
        self.L.cxk_get_order(self.h, _ip(o))
        return o

    def permutation(self):
        n = max(self.num_vars, self.N) + 1
        p = np.zeros(n, dtype=np.int32)
        q = np.zeros(n, dtype=np.int32)
        k = self.L.cxk_get_permutation(self.h, _ip(p), _ip(q))
        return p[:k], q[:k]

    def get_list(self, which, e):
        n = self.L.cxk_get_list(self.h, which, e, None)
        out = np.zeros(max(n, 1), dtype=np.int32)
        self.L.cxk_get_list(self.h, which, e, _ip(out))
        return out[:n]

    def supernode_sizes(self):
        o = np.zeros(self.K, dtype=np.int32)
        self.L.cxk_get_supernode_sizes(self.h, _ip(o))
        return o

    def slab_size(self):
        return self.L.cxk_slab_size(self.h)

    def block_offsets(self):
        d = np.zeros(self.K, dtype=np.int64)
        o = np.zeros(self.K, dtype=np.int64)
        self.L.cxk_get_block_offsets(self.h, _lp(d), _lp(o))
        return d, o

    def ss_index(self, e):
        n = self.L.cxk_get_ss_index(self.h, e, None)
        out = np.zeros(max(n, 1), dtype=np.int64)
        self.L.cxk_get_ss_index(self.h, e, _lp(out))
        return out[:n]

    def num_levels(self):
        return self.L.cxk_num_levels(self.h)

    # ---- numeric
    def set_identity(self):
        self._check(self.L.cxk_set_identity(self.h), "cxk_set_identity")

    def get_W(self, i):
        n = self.L.cxk_dual_size(self.h, i)
        w = np.zeros(max(n, 1))
        self._check(self.L.cxk_get_W(self.h, i, _dp(w)), "cxk_get_W")
        if self.cons[i][0] == "herm":   # (d, n, n) logical planes
            _, order, _, d = self.cons[i]
            return np.transpose(w[:n].reshape(d, order, order), (0, 2, 1)).copy()
        return w[:n]

    def set_W(self, i, w):
        if self.cons[i][0] == "herm":
            w = np.ascontiguousarray(np.swapaxes(np.asarray(w, dtype=np.float64), -1, -2)).ravel()
        else:
            w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).ravel())
        self._check(self.L.cxk_set_W(self.h, i, _dp(w)), "cxk_set_W")

    def assemble(self):
        self._check(self.L.cxk_assemble(self.h), "cxk_assemble")

    def slab(self):
        s = np.zeros(self.slab_size())
        self._check(self.L.cxk_get_slab(self.h, _dp(s)), "cxk_get_slab")
        return s

    def set_slab(self, s):
        s = np.ascontiguousarray(s, dtype=np.float64)
        self._check(self.L.cxk_set_slab(self.h, _dp(s)), "cxk_set_slab")

    def constraint_schur(self, i):
        m = self.cons[i][2]
        G = np.zeros(m * m)
        AW = np.zeros(m)
        AQc = np.zeros(m)
        sc = np.zeros(2)
        self._check(self.L.cxk_get_constraint_schur(self.h, i, _dp(G), _dp(AW), _dp(AQc), _dp(sc)),
                    "cxk_get_constraint_schur")
        return G.reshape(m, m).T.copy(), AW, AQc, sc

    def residuals(self):
        AW = np.zeros(self.span)   # indexed by variable: entries of unused variables stay 0
        AQc = np.zeros(self.span)
        sc = np.zeros(2)
        self._check(self.L.cxk_get_residuals(self.h, _dp(AW), _dp(AQc), _dp(sc)),
                    "cxk_get_residuals")
        return AW, AQc, sc

    def set_refinement(self, iterations):
        """SetIterativeRefinementIterations: takes effect at the next factorization."""
        self._check(self.L.cxk_set_iterative_refinement(self.h, int(iterations)),
                    "cxk_set_iterative_refinement")

    def factor(self):
        ok = C.c_int(0)
        self._check(self.L.cxk_factor(self.h, C.byref(ok)), "cxk_factor")
        return ok.value

    def solve_inplace(self, y):
        y = np.ascontiguousarray(y, dtype=np.float64).ravel().copy()
        if len(y) < self.span:
            raise ValueError(f"solve_inplace: expected {self.span} entries (one per variable and multiplier), got {len(y)}")
        self._check(self.L.cxk_solve_inplace(self.h, _dp(y)), "cxk_solve_inplace")
        return y

    def solve_block(self, Y):
        """Y <- K^-1 Y for a block of right-hand sides with the stored factor (cxk_solve_block).

        A numpy array of shape (N, nrhs), any memory order (1-D: one column), is solved into a new array.
        A torch float64 tensor of shape (N, nrhs) on the context's device is solved IN PLACE through its
        data_ptr() and returned; it must be stored column-major (``t.T.contiguous().T``).  The solve is
        enqueued on the context's stream: when that is not torch's current stream, both are waited for."""
        if hasattr(Y, "data_ptr") and hasattr(Y, "is_contiguous"):
            return self._solve_block_torch(Y)
        Y = np.asarray(Y)
        if Y.dtype.kind not in "fiu":
            raise ValueError(f"solve_block: expected real numbers, got dtype {Y.dtype}")
        one = Y.ndim == 1
        if Y.ndim not in (1, 2):
            raise ValueError(f"solve_block: expected a 1-D or 2-D array, got {Y.ndim} dimensions")
        B = Y.reshape(-1, 1) if one else Y
        if B.shape[0] != self.N or B.shape[1] < 1:
            raise ValueError(f"solve_block: expected shape ({self.N}, nrhs) with nrhs >= 1, got {Y.shape}")
        F = np.array(B, dtype=np.float64, order="F")  # a new array, column-major
        self._check(self.L.cxk_solve_block(self.h, _dp(F), F.shape[0], F.shape[1]), "cxk_solve_block")
        return F[:, 0].copy() if one else F

    def _solve_block_torch(self, t):
        import torch
        if t.dtype != torch.float64:
            raise ValueError(f"solve_block: expected a float64 tensor, got {t.dtype}")
        if not t.is_cuda:
            raise ValueError("solve_block: the tensor must live on the GPU (pass a numpy array for host data)")
        if t.dim() != 2 or t.shape[0] != self.N or t.shape[1] < 1:
            raise ValueError(f"solve_block: expected shape ({self.N}, nrhs) with nrhs >= 1, got {tuple(t.shape)}")
        if t.stride(0) != 1 or (t.shape[1] > 1 and t.stride(1) < t.shape[0]):
            raise ValueError("solve_block: the tensor must be stored column-major (strides (1, ld) with ld >= N), "
                             "for example t.T.contiguous().T")
        ld = int(t.stride(1)) if t.shape[1] > 1 else int(t.shape[0])
        cur = torch.cuda.current_stream(t.device)
        shared = self.stream is not None and int(self.stream) == int(cur.cuda_stream)
        if not shared:
            cur.synchronize()
        self._check(self.L.cxk_solve_block_device(self.h, C.c_void_p(t.data_ptr()), ld, int(t.shape[1])),
                    "cxk_solve_block_device")
        if not shared:
            self.sync()
        return t

    def set_cost(self, b):
        b = np.ascontiguousarray(np.asarray(b, dtype=np.float64).ravel())
        self._check(self.L.cxk_set_cost(self.h, _dp(b)), "cxk_set_cost")

    def newton_direction(self, inv_sqrt_mu, b_scaling=1.0, c_scaling=1.0):
        self._check(self.L.cxk_newton_direction(self.h, inv_sqrt_mu, b_scaling, c_scaling),
                    "cxk_newton_direction")

    def factor_solve_async(self, cb, cq, cw):
        """Factor and solve y <- K^-1 (cb b + cq AQc + cw AW) in one upward pass (cxk_factor_solve_async)."""
        self._check(self.L.cxk_factor_solve_async(self.h, cb, cq, cw), "cxk_factor_solve_async")

    def factor_direction_async(self, inv_sqrt_mu, b_scaling=1.0, c_scaling=1.0):
        self._check(self.L.cxk_factor_direction_async(self.h, inv_sqrt_mu, b_scaling, c_scaling),
                    "cxk_factor_direction_async")

    def solve_rhs(self, cb, cq, cw):
        self._check(self.L.cxk_solve_rhs(self.h, cb, cq, cw), "cxk_solve_rhs")

    def step_scalars(self):
        out = np.zeros(6)
        self._check(self.L.cxk_step_scalars(self.h, _dp(out)), "cxk_step_scalars")
        return out

    def factor_status(self):
        """1 when the latest factorization succeeded (cxk_factor_status)."""
        ok = C.c_int(0)
        self._check(self.L.cxk_factor_status(self.h, C.byref(ok)), "cxk_factor_status")
        return ok.value

    def kkt_solve_async(self, inv_sqrt_mu, b_scaling=1.0, c_scaling=1.0):
        self._check(self.L.cxk_kkt_solve_async(self.h, inv_sqrt_mu, b_scaling, c_scaling),
                    "cxk_kkt_solve_async")

    def sync(self):
        ok = C.c_int(0)
        self._check(self.L.cxk_sync(self.h, C.byref(ok)), "cxk_sync")
        return ok.value

    def kkt_solve(self, b, inv_sqrt_mu, b_scaling=1.0, c_scaling=1.0):
        self.set_cost(b)
        self.kkt_solve_async(inv_sqrt_mu, b_scaling, c_scaling)
        ok = self.sync()
        return ok, self.get_y()

    def get_y(self):
        y = np.zeros(self.span)   # indexed by variable: entries of unused variables stay 0
        self._check(self.L.cxk_get_y(self.h, _dp(y)), "cxk_get_y")
        return y

    def set_y(self, y):
        y = np.ascontiguousarray(y, dtype=np.float64).ravel()
        if len(y) < self.span:
            raise ValueError(f"set_y: expected {self.span} entries (one per variable and multiplier), got {len(y)}")
        self._check(self.L.cxk_set_y(self.h, _dp(y)), "cxk_set_y")

    def prepare_step(self, y, c_weight, e_weight=1.0, affine=0):
        if y is not None:
            self.set_y(y)
        info = np.zeros(2)
        self._check(self.L.cxk_prepare_step(self.h, affine, c_weight, e_weight, _dp(info)),
                    "cxk_prepare_step")
        return info

    def prepare_take_step(self, y, c_weight, e_weight=1.0):
        """PrepareStep + TakeStep with the step length min(1, 2 / norminfd^2) evaluated on the device
        (cxk_prepare_take_step) -> (normsqrd, norminfd, took)."""
        if y is not None:
            self.set_y(y)
        info = np.zeros(2)
        took = C.c_int(0)
        self._check(self.L.cxk_prepare_take_step(self.h, c_weight, e_weight, _dp(info), C.byref(took)),
                    "cxk_prepare_take_step")
        return info[0], info[1], bool(took.value)

    def take_step(self, step_size, e_weight=1.0, affine=0):
        self._check(self.L.cxk_take_step(self.h, affine, e_weight, step_size), "cxk_take_step")

    def line_search(self, dinf_upper_bound, b_scaling=1.0, c_scaling=1.0):
        """ComputeMuFromLineSearch with the current factorization and cost (cxk_line_search): the admissible
        inv_sqrt_mu, or -1 (an empty interval, or a cone without line-search support).  Overwrites y."""
        out = np.zeros(1)
        self._check(self.L.cxk_line_search(self.h, dinf_upper_bound, b_scaling, c_scaling, _dp(out)),
                    "cxk_line_search")
        return float(out[0])

    def weighted_slack_eigenvalues(self, y, c_weight):
        if y is not None:
            self.set_y(y)
        out = np.zeros(4)
        self._check(self.L.cxk_weighted_slack_eigenvalues(self.h, c_weight, _dp(out)),
                    "cxk_weighted_slack_eigenvalues")
        return out

    # ---- multi-GPU exchange / accounting
    def exchange_buffer(self):
        p = C.c_void_p()
        n = C.c_long()
        self._check(self.L.cxk_exchange_buffer(self.h, C.byref(p), C.byref(n)),
                    "cxk_exchange_buffer")
        return p.value, n.value

    def kkt_local_async(self, inv_sqrt_mu, b_scaling=1.0, c_scaling=1.0):
        self._check(self.L.cxk_kkt_local_async(self.h, inv_sqrt_mu, b_scaling, c_scaling),
                    "cxk_kkt_local_async")

    def kkt_finish_async(self, inv_sqrt_mu, b_scaling=1.0, c_scaling=1.0):
        self._check(self.L.cxk_kkt_finish_async(self.h, inv_sqrt_mu, b_scaling, c_scaling),
                    "cxk_kkt_finish_async")

    def set_solver_mode(self, mode):
        """0 / 1 supernodal LLT / LDLT (by structure), 2 dense column-pivoted QR (cxk_set_solver_mode)."""
        self._check(self.L.cxk_set_solver_mode(self.h, mode), "cxk_set_solver_mode")

    def phase_timers(self, on=True):
        self._check(self.L.cxk_phase_timers(self.h, int(bool(on))), "cxk_phase_timers")

    def phase_mark(self, phase):
        self._check(self.L.cxk_phase_mark(self.h, phase), "cxk_phase_mark")

    def phase_read(self, reset=False):
        out = np.zeros(5)
        self._check(self.L.cxk_phase_read(self.h, _dp(out), int(bool(reset))), "cxk_phase_read")
        return out

    # ---- collectives of a sharded context (cxk_comm_*)
    @staticmethod
    def comm_unique_id():
        """ncclGetUniqueId: 128 bytes made by ONE rank and handed to all (cxk_comm_unique_id)."""
        buf = C.create_string_buffer(128)
        if load_library().cxk_comm_unique_id(buf) != 0:
            raise KktError("cxk_comm_unique_id failed (librccl.so missing?)")
        return buf.raw

    def comm_init_rccl(self, unique_id, rank, world):
        """RCCL communicator for this context's device; before initialize() it also sets the shard."""
        assert len(unique_id) == 128
        self._check(self.L.cxk_comm_init_rccl(self.h, C.c_char_p(unique_id), rank, world), "cxk_comm_init_rccl")

    def comm_init_rccl_solo(self):
        """Diagnostic: one-rank RCCL communicator under a larger virtual shard world (cxk_comm_init_rccl_solo)."""
        self._check(self.L.cxk_comm_init_rccl_solo(self.h), "cxk_comm_init_rccl_solo")

    def comm_count(self):
        """Ranks the attached RCCL communicator holds (ncclCommCount); 0 without one."""
        return int(self.L.cxk_comm_count(self.h))

    def comm_selftest(self, count=1000):
        self._check(self.L.cxk_comm_selftest(self.h, count), "cxk_comm_selftest")

    def comm_set_allreduce(self, host_allreduce):
        """Another transport / tests: host_allreduce(array, op) -> array reduces HOST copies across the
        ranks (op 0 sum, 1 max, 2 min); the wrapper moves the device buffer to the host and back."""
        hip = C.CDLL("libamdhip64.so")
        fn_t = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p)

        def _cb(user, dev, count, op, stream):
            try:
                buf = np.empty(count)
                if hip.hipStreamSynchronize(C.c_void_p(stream)) != 0:
                    return 1
                if hip.hipMemcpy(buf.ctypes.data_as(C.c_void_p), C.c_void_p(dev), C.c_size_t(8 * count), 2) != 0:
                    return 1
                out = np.ascontiguousarray(host_allreduce(buf, op), dtype=np.float64)
                if hip.hipMemcpy(C.c_void_p(dev), out.ctypes.data_as(C.c_void_p), C.c_size_t(8 * count), 1) != 0:
                    return 1
                return 0
            except Exception:  # an exception must not cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        self._coll_cb = fn_t(_cb)  # keeps the trampoline alive as long as the context
        self._check(self.L.cxk_comm_set_allreduce(self.h, C.cast(self._coll_cb, C.c_void_p), None),
                    "cxk_comm_set_allreduce")

    def owns(self, i):
        return bool(self.L.cxk_owns_constraint(self.h, i))

    def valid_variables(self):
        m = np.zeros(self.span, dtype=np.uint8)   # indexed by variable: unused variables are not valid
        self._check(self.L.cxk_get_valid_variables(self.h, m.ctypes.data_as(C.POINTER(C.c_ubyte))),
                    "cxk_get_valid_variables")
        return m.astype(bool)

    def shard_info(self):
        cut, nlev, cnt = C.c_int(), C.c_int(), C.c_long()
        self._check(self.L.cxk_shard_info(self.h, C.byref(cut), C.byref(nlev), C.byref(cnt)),
                    "cxk_shard_info")
        return cut.value, nlev.value, cnt.value

    def exchange_download(self):
        _, count = self.exchange_buffer()
        out = np.zeros(count)
        self._check(self.L.cxk_exchange_download(self.h, _dp(out)), "cxk_exchange_download")
        return out

    def exchange_upload(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        self._check(self.L.cxk_exchange_upload(self.h, _dp(x)), "cxk_exchange_upload")

    def exchange_tensor(self, torch):
        """Zero-copy torch view of the device exchange buffer (for torch.distributed.all_reduce)."""
        ptr, count = self.exchange_buffer()

        class _Arr:
            __cuda_array_interface__ = {"shape": (count,), "typestr": "<f8", "data": (ptr, False),
                                        "version": 2}
        return torch.as_tensor(_Arr(), device="cuda")

    def assemble_local(self):
        self._check(self.L.cxk_assemble_local(self.h), "cxk_assemble_local")

    def finish_assemble(self):
        self._check(self.L.cxk_finish_assemble(self.h), "cxk_finish_assemble")

    def dense_top_columns(self):
        """Columns factored by the dense top kernel (cxk_dense_top_columns); 0 when it is not used."""
        return self.L.cxk_dense_top_columns(self.h)

    def count_sparse_lmi(self):
        """Constraints on the sparse-LMI evaluation path (cxk_count_sparse_lmi)."""
        return self.L.cxk_count_sparse_lmi(self.h)

    def fused_assembly(self):
        """True when the assembly rides in the first factor level's launch (cxk_fused_assembly)."""
        return bool(self.L.cxk_fused_assembly(self.h))

    def fused_tree(self):
        """True when a KKT solve runs as one launch over the whole elimination tree (cxk_fused_tree)."""
        return bool(self.L.cxk_fused_tree(self.h))

    def fused_tree_frames(self):
        """((NSMAX, SMAX), (NSMAX, SMAX)): the pair of register frames of the whole-tree launch (cxk_fused_tree_frames)."""
        fn = self.L.cxk_fused_tree_frames
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        a, b = C.c_int(0), C.c_int(0)
        self._check(fn(self.h, C.byref(a), C.byref(b)), "cxk_fused_tree_frames")
        return (a.value >> 8, a.value & 255), (b.value >> 8, b.value & 255)

    def count_lmi_kernel(self, which):
        """Constraints whose Schur block comes from kernel `which` (cxk_count_lmi_kernel): 0 literal,
        1 DPP + MFMA rows, 2 persistent MFMA, 3 GEMM pipeline, 4 sparse."""
        return self.L.cxk_count_lmi_kernel(self.h, which)

    def lmi_kernels(self, i):
        """{stage: kernel instance name} of LMI / Hermitian constraint i (cxk_lmi_kernels)."""
        out = (C.c_int * 5)()
        self._check(self.L.cxk_lmi_kernels(self.h, i, out), "cxk_lmi_kernels")
        return {s: self.L.cxk_lmi_kernel_name(out[j]).decode() for j, s in enumerate(LMI_STAGES)}

    def step_info(self):
        """Per-constraint (normsqrd, norminfd) of the last prepare_step, shape (K, 2) (cxk_get_step_info)."""
        out = np.zeros(2 * self.K)
        self._check(self.L.cxk_get_step_info(self.h, _dp(out)), "cxk_get_step_info")
        return out.reshape(self.K, 2)

    def assembly_work(self):
        b = C.c_double()
        f = C.c_double()
        self.L.cxk_assembly_work(self.h, C.byref(b), C.byref(f))
        return b.value, f.value

    def enable_timing(self, on=True):
        self.L.cxk_enable_timing(self.h, int(on))

    def kernel_time(self, reset=True):
        ms = C.c_double()
        n = self.L.cxk_kernel_time(self.h, int(reset), C.byref(ms))
        return n, ms.value

    CLOCKS = {"assembly": 0, "tree": 1, "solve": 2, "query": 3, "prepare": 4, "take": 5}

    def kernel_clock(self, which, reset=True):
        """(samples, average ms) of a kernel clock slot (cxk_kernel_clock; names in CLOCKS)."""
        ms = C.c_double()
        n = self.L.cxk_kernel_clock(self.h, self.CLOCKS[which] if isinstance(which, str) else int(which),
                                    int(reset), C.byref(ms))
        return n, ms.value

    def set_chain_segments(self, segments):
        """0: the reference's elimination order; P >= 2: a chain-shaped tree in P segments (before initialize)."""
        self._check(self.L.cxk_set_chain_segments(self.h, int(segments)), "cxk_set_chain_segments")

    def chain_segments(self):
        return self.L.cxk_chain_segments(self.h)

    def set_streamed_cones(self, on=True):
        """Second-order cones larger than LDS are held in HBM and run by the streamed kernels instead of being
        refused at initialize (before initialize; default: CXK_STREAMED_CONES in the environment, else refused)."""
        self._check(self.L.cxk_set_streamed_cones(self.h, int(bool(on))), "cxk_set_streamed_cones")

    def count_streamed_cones(self):
        """Constraints this context owns that run on the streamed second-order cone kernels."""
        return self.L.cxk_count_streamed_cones(self.h)

    def set_streamed_quadratic(self, mode=1):
        """Quadratic cones held in HBM on the streamed kernels: 1 every cone, 0 none (a cone beyond LDS is then refused
        at initialize), -1 those beyond LDS and those large enough to be faster there (before initialize; default:
        CXK_STREAMED_QUADRATIC in the environment, else 0)."""
        self._check(self.L.cxk_set_streamed_quadratic(self.h, int(mode)), "cxk_set_streamed_quadratic")

    def count_streamed_quadratic(self):
        """Constraints this context owns that run on the streamed quadratic cone kernels."""
        return self.L.cxk_count_streamed_quadratic(self.h)

    def set_tiled_linear(self, mode=1):
        """Linear blocks on the tiled kernels: 1 every block, 0 none (a block over more than 4096 variables is then
        refused at initialize), -1 by size (before initialize; default: CXK_TILED_LINEAR in the environment, else -1)."""
        self._check(self.L.cxk_set_tiled_linear(self.h, int(mode)), "cxk_set_tiled_linear")

    def count_tiled_linear(self):
        """Constraints this context owns that run on the tiled linear kernels."""
        return self.L.cxk_count_tiled_linear(self.h)

    def set_sparse_linear(self, mode=1):
        """Linear blocks evaluated from their nonzeros: 1 every block, 0 none, -1 those whose pattern makes it pay
        (before initialize; default: CXK_SPARSE_LINEAR in the environment, else 0)."""
        self._check(self.L.cxk_set_sparse_linear(self.h, int(mode)), "cxk_set_sparse_linear")

    def count_sparse_linear(self):
        """Constraints this context owns that run on the sparse linear kernels."""
        return self.L.cxk_count_sparse_linear(self.h)

    def set_sparse_soc(self, mode=1):
        """Second-order cones evaluated from their nonzeros: 1 every cone, 0 none, -1 those that can run nowhere else or
        whose pattern makes it pay (before initialize; default: CXK_SPARSE_SOC in the environment, else 0)."""
        self._check(self.L.cxk_set_sparse_soc(self.h, int(mode)), "cxk_set_sparse_soc")

    def count_sparse_soc(self):
        """Constraints this context owns that run on the sparse second-order-cone kernels."""
        return self.L.cxk_count_sparse_soc(self.h)

    def set_sparse_affine(self, mode=1):
        """The affine term of sparse matrix inequalities of order 64 and up, when it has more than 64 nonzeros: 1 from
        its nonzeros, 0 by two dense products, -1 from its nonzeros when that pays (before initialize; default:
        CXK_SPARSE_AFFINE in the environment, else 0 for add_lmi / add_hermitian and -1 for add_lmi_coo)."""
        self._check(self.L.cxk_set_sparse_affine(self.h, int(mode)), "cxk_set_sparse_affine")

    def count_sparse_affine(self):
        """Constraints this context owns whose affine term is evaluated from its nonzeros."""
        return self.L.cxk_count_sparse_affine(self.h)

    def set_sparse_fold(self, mode=1):
        """The sums of sparse Hermitian matrix inequalities over C or H: 1 over the top block row of the real
        representations (a d-th of the terms), 0 over all of it (before initialize; default: CXK_SPARSE_FOLD in the
        environment, else 0 for add_hermitian and 1 for add_hermitian_coo)."""
        self._check(self.L.cxk_set_sparse_fold(self.h, int(mode)), "cxk_set_sparse_fold")

    def count_sparse_fold(self):
        """Constraints this context owns that run on the folded sparse kernels."""
        return self.L.cxk_count_sparse_fold(self.h)

    def set_wide_spectrum(self, mode=1):
        """The Lanczos run of large-order matrix inequalities spread over the chip: 1 every large-order group, 0 none
        (orders above 2549 are then refused), -1 only the orders the one-workgroup run cannot hold (before initialize;
        default: CXK_WIDE_SPECTRUM in the environment, else -1)."""
        self._check(self.L.cxk_set_wide_spectrum(self.h, int(mode)), "cxk_set_wide_spectrum")

    def count_wide_spectrum(self):
        """Constraints this context owns whose Lanczos runs take the chip-wide kernels."""
        return self.L.cxk_count_wide_spectrum(self.h)

    def count_factored_lmi(self):
        """Constraints this context owns that were added by add_lmi_factored or add_hermitian_factored
        (kernels_lmi_factored.hip.h)."""
        return self.L.cxk_count_factored_lmi(self.h)

    def sparse_soc_setup_ms(self):
        """Device milliseconds initialize() spent forming the constants H, h, z of the sparse second-order cones."""
        return self.L.cxk_sparse_soc_setup_ms(self.h)

    def fused_tree_timed_out(self):
        return bool(self.L.cxk_fused_tree_timed_out(self.h))

    def debug_force_fused_timeout(self):
        self._check(self.L.cxk_debug_force_fused_timeout(self.h), "cxk_debug_force_fused_timeout")

    # cxk_debug_fused_timeout_at's sites
    DEBUG_FUSED_FACTOR, DEBUG_FUSED_SHARD_UP, DEBUG_FUSED_SHARD_TOP, DEBUG_FUSED_STREAM_ORDERED = 0, 1, 2, 16

    def debug_fused_timeout_at(self, launch_index, which):
        """Test hook: the launch_index-th whole-tree factor launch from now reports a wait that ran out
        behind its launch `which` (DEBUG_FUSED_*)."""
        self._check(self.L.cxk_debug_fused_timeout_at(self.h, launch_index, which), "cxk_debug_fused_timeout_at")


def gemm_f64(A, B, C=None, ta=False, tb=False, alpha=1.0, beta=0.0, lower_only=False, splits=1,
             reps=1, device=0):
    """Batched C = alpha op(A) op(B) + beta C through cxk_gemm_f64 (fp64 MFMA kernel).

    A: (batch, M, K) logical operand op(A); B: (batch, K, N); returns (C, avg_ms).  The packed
    column-major buffers the C-ABI expects are built here (ta / tb choose the stored layout)."""
    import ctypes as C_
    L = load_library()
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    batch, M, K = A.shape
    N = B.shape[2]
    # stored A: M x K column-major (ta False) or K x M column-major (ta True)
    Ap = np.ascontiguousarray(A if ta else A.transpose(0, 2, 1))     # col-major(MxK) == C-order(KxM)
    Bp = np.ascontiguousarray(B.transpose(0, 2, 1) if not tb else B)  # stored K x N col-major, or N x K
    Cp = np.zeros((batch, N, M)) if C is None else np.ascontiguousarray(
        np.asarray(C, dtype=np.float64).transpose(0, 2, 1))
    ms = C_.c_double(0.0)
    L.cxk_gemm_f64.restype = C_.c_int
    L.cxk_gemm_f64.argtypes = [C_.c_int] * 7 + [C_.c_void_p] * 3 + [C_.c_double] * 2 + [C_.c_int] * 3 + [
        C_.POINTER(C_.c_double)]
    rc = L.cxk_gemm_f64(device, int(ta), int(tb), M, N, K, batch, Ap.ctypes.data, Bp.ctypes.data,
                        Cp.ctypes.data, alpha, beta, int(lower_only), splits, reps, C_.byref(ms))
    if rc != 0:
        raise RuntimeError("cxk_gemm_f64 failed")
    return Cp.transpose(0, 2, 1).copy(), ms.value


# cxk_gemm_f64_layout: the route enumerators and the order of the call's fields (include/conex_kkt_hip.h)
GEMM_ROUTES = ("general", "dma16", "dma32", "dma128x128", "dma128x64")
GEMM_LAYOUT_FIELDS = ("M", "N", "K", "ta", "tb", "batch", "inner", "lower_only", "splits", "ordered", "tile", "general",
                      "offA", "lda", "sA1", "sA2", "offB", "ldb", "sB1", "sB2", "offC", "ldc", "sC1", "sC2",
                      "offCt", "ldct", "sT1", "sT2", "ctb", "sTb", "offPart", "sCs")


def gemm_f64_layout(arena, fields, alpha=1.0, beta=0.0, device=0):
    """One product through cxk_gemm_f64_layout on operands that live inside `arena` (1-d float64) at the element
    offsets, leading dimensions and strides `fields` states (a dict over GEMM_LAYOUT_FIELDS; offCt / offPart
    default to -1 = none, everything else to 0, inner / splits / ordered to 1).  Returns (arena after the call, name
    of the route the call ran on).  A layout that leaves the arena raises before anything is launched."""
    import ctypes as C_
    L = load_library()
    arena = np.ascontiguousarray(arena, dtype=np.float64)
    if arena.ndim != 1:
        raise ValueError("arena must be one-dimensional")
    unknown = set(fields) - set(GEMM_LAYOUT_FIELDS)
    if unknown:
        raise ValueError("unknown layout fields: %s" % sorted(unknown))
    default = {"offCt": -1, "offPart": -1, "inner": 1, "splits": 1, "ordered": 1}
    f = (C_.c_longlong * len(GEMM_LAYOUT_FIELDS))(*[int(fields.get(k, default.get(k, 0))) for k in GEMM_LAYOUT_FIELDS])
    out = arena.copy()
    route = C_.c_int(-1)
    L.cxk_gemm_f64_layout.restype = C_.c_int
    L.cxk_gemm_f64_layout.argtypes = [C_.c_int, C_.c_void_p, C_.c_longlong, C_.POINTER(C_.c_longlong), C_.c_double,
                                      C_.c_double, C_.POINTER(C_.c_int)]
    rc = L.cxk_gemm_f64_layout(device, out.ctypes.data, out.size, f, float(alpha), float(beta), C_.byref(route))
    if rc != 0:
        raise RuntimeError("cxk_gemm_f64_layout refused the layout or failed")
    return out, GEMM_ROUTES[route.value]
