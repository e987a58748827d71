"""Python-3 front end with the surface of the reference's ``ConexProgram.Conex`` class
(interfaces/python/ConexProgram.py:58-277, Python 2 over a SWIG module), on ctypes over
``libconex.so``'s ``CONEX_*`` ABI (include/conex.h) -- so every solve runs the HIP path.

Conventions kept from the reference wrapper:

* matrix inequalities are passed as an ``n x n x m`` array, ``A[:, :, i]`` multiplying variable
  ``i`` (the SWIG typemap takes Fortran-ordered 3-D input, conex.i:17-29), and the constraint is
  ``c - sum_i y_i A[:, :, i]  >= 0``;
* ``Maximize(b)`` / ``Solve()`` return a :class:`Solution` with ``y`` and ``status`` (1 = solved,
  the polarity of cone_program.cc:532);
* builder failures raise (the reference raises ``NameError``; here :class:`ConexError`, a subclass);
* ``DefaultConfiguration`` applies the wrapper's own overrides (ConexProgram.py:115-125) on top of
  ``CONEX_SetDefaultOptions``.

Arrays are plain ``numpy.ndarray`` (the reference uses ``numpy.matrix``).
"""
import ctypes as C

import numpy as np

from . import capi


class ConexError(NameError):
    """Raised where the reference wrapper raises NameError."""


class Errors:
    """Optimality measures of :meth:`Conex.ComputeErrors` (ConexProgram.py:11-15, 244-277)."""

    def __init__(self):
        self.Ax_minus_b = 0.0
        self.x_dot_s = 0.0
        self.min_eig_S = []
        self.min_eig_X = []


class Solution:
    def __init__(self):
        self.err = Errors()
        self.x = []
        self.y = []
        self.s = []
        self.status = 0


class LMIOperator:
    """y -> sum_i y[var_i] A[:, :, i]  and its adjoint  X -> (tr(A[:, :, i] X))_i."""

    def __init__(self, matrices, num_vars=None, variables=None):
        self.matrices = np.asarray(matrices, dtype=np.float64)
        m_local = self.matrices.shape[2]
        self.variables = list(range(m_local)) if variables is None else [int(v) for v in variables]
        if len(self.variables) != m_local:
            raise ConexError("Invalid LMI")
        self.m = m_local if num_vars is None else int(num_vars)

    def apply(self, y):
        y = np.asarray(y, dtype=np.float64).ravel()
        out = np.zeros(self.matrices.shape[:2])
        for i, var in enumerate(self.variables):
            out += self.matrices[:, :, i] * y[var]
        return out

    def adjoint(self, X):
        out = np.zeros(self.m)
        for i, var in enumerate(self.variables):
            out[var] += np.trace(self.matrices[:, :, i] @ np.asarray(X))
        return out


class _LinearOperator:
    def __init__(self, A):
        self.A = np.asarray(A, dtype=np.float64)
        self.m = self.A.shape[1]

    def apply(self, y):
        return self.A @ np.asarray(y, dtype=np.float64).ravel()

    def adjoint(self, x):
        return self.A.T @ np.asarray(x, dtype=np.float64).ravel()


class _FactoredLMIOperator:
    """y -> sum_i y_i A_i with A_i = sum_k sigma_k f_k f_k', k in rank_ptr[i]:rank_ptr[i + 1], and its adjoint, from the
    factors (the matrices are never formed)."""

    def __init__(self, F, rank_ptr, sigma, num_vars, variables):
        self.F, self.sigma = F, sigma
        self.var = np.repeat(np.arange(len(rank_ptr) - 1), np.diff(rank_ptr))
        self.m = num_vars
        self.variables = np.arange(len(rank_ptr) - 1) if variables is None else np.asarray(variables, dtype=np.int64)

    def apply(self, y):
        y = np.asarray(y, dtype=np.float64).ravel()[self.variables]
        return (self.F * (self.sigma * y[self.var])) @ self.F.T

    def adjoint(self, X):
        out = np.zeros(self.m)
        np.add.at(out, self.variables[self.var], self.sigma * np.einsum("ak,ab,bk->k", self.F, np.asarray(X), self.F))
        return out


class _EntriesLMIOperator:
    """y -> sum_i y_i A_i and its adjoint for matrices given by the entries of their lower triangles (never formed
    one by one; apply returns the n x n sum)."""

    def __init__(self, n, ptr, row, col, val, num_vars, variables):
        m = len(ptr) - 2
        self.n, self.m = n, num_vars
        self.row, self.col, self.val = row[:ptr[m]], col[:ptr[m]], val[:ptr[m]]
        self.var = np.repeat(np.arange(m), np.diff(ptr[:m + 1]))
        self.variables = np.arange(m) if variables is None else np.asarray(variables, dtype=np.int64)

    def apply(self, y):
        y = np.asarray(y, dtype=np.float64).ravel()[self.variables]
        out = np.zeros((self.n, self.n))
        w = self.val * y[self.var]
        np.add.at(out, (self.row, self.col), w)
        off = self.row != self.col
        np.add.at(out, (self.col[off], self.row[off]), w[off])
        return out

    def adjoint(self, X):
        X = np.asarray(X)
        t = self.val * np.where(self.row == self.col, X[self.row, self.col], X[self.row, self.col] + X[self.col, self.row])
        out = np.zeros(self.m)
        np.add.at(out, self.variables[self.var], t)
        return out


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


class Conex:
    def __init__(self, m=-1):
        self._L = capi.api()
        self.a = self._L.CONEX_CreateConeProgram()
        if m >= 0 and self._L.CONEX_SetNumberOfVariables(self.a, int(m)) != 0:
            raise ConexError("Failed to set the number of variables.")
        self.num_constraints = 0
        self.A = []   # operators of the constraints added through the Add* calls
        self.c = []   # their affine terms (shape = shape of the dual variable)
        self.m = m

    def __del__(self):
        if getattr(self, "a", None):
            self._L.CONEX_DeleteConeProgram(self.a)
            self.a = None

    # ---- options and statistics
    def DefaultConfiguration(self):
        cfg = capi.default_config()
        cfg.inv_sqrt_mu_max = 1000
        cfg.maximum_mu = 1e20
        cfg.max_iterations = 100
        cfg.final_centering_steps = 1
        cfg.prepare_dual_variables = 1
        cfg.infeasibility_threshold = 1e8
        cfg.divergence_upper_bound = 1
        return cfg

    def GetIterationNumberStats(self, num):
        st = capi.IterationStats()
        self._L.CONEX_GetIterationStats(self.a, C.byref(st), int(num))
        return st

    def GetIterationStats(self):
        last = self.GetIterationNumberStats(-1).iteration_number
        return [self.GetIterationNumberStats(i) for i in range(last + 1)]

    # ---- whole-constraint builders
    def AddLinearInequality(self, A, c):
        A = np.asarray(A, dtype=np.float64)
        c = np.asarray(c, dtype=np.float64).ravel()
        Af = capi.colmajor(A)
        if self._L.CONEX_AddDenseLinearConstraint(self.a, capi.dp(Af), A.shape[0], A.shape[1],
                                                  capi.dp(_f64(c)), len(c)) < 0:
            raise ConexError("Failed to add constraint.")
        self.m = A.shape[1]
        self.A.append(_LinearOperator(A))
        self.c.append(c.copy())
        self.num_constraints += 1

    def AddLinearInequalities(self, A, lb, ub):
        A = np.asarray(A, dtype=np.float64)
        lb = _f64(np.asarray(lb, dtype=np.float64).ravel())
        ub = _f64(np.asarray(ub, dtype=np.float64).ravel())
        Af = capi.colmajor(A)
        self._L.CONEX_AddLinearInequalities(self.a, capi.dp(Af), A.shape[0], A.shape[1], capi.dp(lb), len(lb),
                                            capi.dp(ub), len(ub))
        self.A.append(_LinearOperator(A))
        self.c.append(ub.copy())
        self.num_constraints += 1

    def AddQuadraticCost(self, P):
        P = np.asarray(P, dtype=np.float64)
        if P.shape[0] != self.m or P.shape[1] != self.m:
            raise ConexError("Cost matrix dimension does not match number of variables.")
        Pf = capi.colmajor(P)
        self._L.CONEX_AddQuadraticCost(self.a, capi.dp(Pf), P.shape[0], P.shape[1])

    def _lmi_buffers(self, A, c):
        A = np.asarray(A, dtype=np.float64)
        c = np.asarray(c, dtype=np.float64)
        if A.ndim != 3 or A.shape[0] != A.shape[1] or c.shape != A.shape[:2]:
            raise ConexError("Invalid LMI")
        Af = np.ascontiguousarray(np.transpose(A, (2, 1, 0))).ravel()  # [i][col][row]: column-major n x n x m
        return A, c, Af, capi.colmajor(c)

    def AddDenseLinearMatrixInequality(self, A, c):
        A, c, Af, cf = self._lmi_buffers(A, c)
        n, m = A.shape[0], A.shape[2]
        if self._L.CONEX_AddDenseLMIConstraint(self.a, capi.dp(Af), n, n, m, capi.dp(cf), n, n) < 0:
            raise ConexError("Failed to add constraint.")
        self.n, self.m = n, m
        self.A.append(LMIOperator(A))
        self.c.append(c.copy())
        self.num_constraints += 1

    def AddSparseLinearMatrixInequality(self, A, c, variables):
        variables = np.asarray(variables).astype(np.int64).ravel()
        if len(variables) and int(variables.max()) + 1 > self.m:
            raise ConexError("Invalid sparse LMI. %d != %d" % (self.m, int(variables.max()) + 1))
        A, c, Af, cf = self._lmi_buffers(A, c)
        n, m = A.shape[0], A.shape[2]
        v = np.ascontiguousarray(variables, dtype=np.int64)
        if self._L.CONEX_AddSparseLMIConstraint(self.a, capi.dp(Af), n, n, m, capi.dp(cf), n, n,
                                                v.ctypes.data_as(C.POINTER(C.c_long)), len(v)) < 0:
            raise ConexError("Failed to add constraint.")
        self.A.append(LMIOperator(A, self.m, variables))
        self.c.append(c.copy())
        self.num_constraints += 1

    def AddFactoredLinearMatrixInequality(self, F, rank_ptr, sigma, c, variables=None):
        """c - sum_i y_i A_i positive semidefinite with low-rank A_i = sum_k sigma[k] F[:, k] F[:, k]',
        k in rank_ptr[i]:rank_ptr[i + 1], given by its factors and never expanded (CONEX_HIP_AddFactoredLMIConstraint,
        an extra next to the reference's surface).  F is n x R, rank_ptr has one entry more than the constraint has
        variables (len(variables), or all when None), sigma R entries or None (all +1), c is n x n symmetric.
        Returns the constraint id."""
        c = np.asarray(c, dtype=np.float64)
        if c.ndim != 2 or c.shape[0] != c.shape[1]:
            raise ConexError("Invalid LMI")
        n = c.shape[0]
        F = np.asarray(F, dtype=np.float64).reshape(n, -1)
        rp = np.ascontiguousarray(np.asarray(rank_ptr).ravel(), dtype=np.int32)
        R = F.shape[1]
        sg = np.ones(R) if sigma is None else _f64(np.asarray(sigma, dtype=np.float64).ravel())
        if len(rp) < 1 or len(sg) != R:
            raise ConexError("Invalid LMI")
        v = None if variables is None else np.ascontiguousarray(np.asarray(variables).ravel(), dtype=np.int64)
        if len(rp) - 1 != (self.m if v is None else len(v)):
            raise ConexError("Invalid LMI")
        Ff, cf = capi.colmajor(F), capi.colmajor(c)
        cid = self._L.CONEX_HIP_AddFactoredLMIConstraint(
            self.a, n, capi.dp(Ff), R, capi.dp(sg), rp.ctypes.data_as(C.POINTER(C.c_int)), len(rp) - 1, capi.dp(cf),
            None if v is None else v.ctypes.data_as(C.POINTER(C.c_long)))
        if cid < 0:
            raise ConexError("Failed to add constraint.")
        self.A.append(_FactoredLMIOperator(F, rp, sg, self.m, v))
        self.c.append(c.copy())
        self.num_constraints += 1
        return cid

    def AddLinearMatrixInequalityFromEntries(self, n, ptr, row, col, val, variables=None):
        """c - sum_i y_i A_i positive semidefinite of order n with sparse symmetric A_i and c given by the entries of
        their lower triangles and never expanded (CONEX_HIP_AddLMIConstraintFromEntries, an extra next to the reference's
        surface): list i, ptr[i]:ptr[i + 1] of row / col / val with row >= col, holds A_i, the last list holds c; ptr has
        two entries more than the constraint has variables (len(variables), or all when None).  Entries of a list come
        in any order, explicit zeros are dropped, an empty list is the zero matrix.  UpdateLinearOperator and
        UpdateAffineTerm fail on such a constraint.  Returns the constraint id."""
        pt = np.ascontiguousarray(np.asarray(ptr).ravel(), dtype=np.int32)
        rw = np.ascontiguousarray(np.asarray(row).ravel(), dtype=np.int32)
        cl = np.ascontiguousarray(np.asarray(col).ravel(), dtype=np.int32)
        vl = _f64(np.asarray(val, dtype=np.float64).ravel())
        v = None if variables is None else np.ascontiguousarray(np.asarray(variables).ravel(), dtype=np.int64)
        m = self.m if v is None else len(v)
        if n < 1 or len(pt) != m + 2 or not (len(rw) == len(cl) == len(vl)) or pt[-1] > len(vl) or np.any(np.diff(pt) < 0):
            raise ConexError("Invalid LMI")
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        cid = self._L.CONEX_HIP_AddLMIConstraintFromEntries(
            self.a, int(n), ip(pt), ip(rw), ip(cl), capi.dp(vl), m, None if v is None else v.ctypes.data_as(C.POINTER(C.c_long)))
        if cid < 0:
            raise ConexError("Failed to add constraint.")
        self.A.append(_EntriesLMIOperator(int(n), pt, rw, cl, vl, self.m, v))
        c = np.zeros((int(n), int(n)))
        cs = slice(pt[m], pt[m + 1])
        c[rw[cs], cl[cs]] = vl[cs]
        c[cl[cs], rw[cs]] = vl[cs]
        self.c.append(c)
        self.num_constraints += 1
        return cid

    def SetSparseAffine(self, mode):
        """How sparse matrix inequalities of order 64 and up evaluate an affine term of more than 64 nonzeros: 1 from
        its nonzeros, 0 by two dense products, -1 from its nonzeros when that pays (CONEX_HIP_SetSparseAffine)."""
        if self._L.CONEX_HIP_SetSparseAffine(self.a, int(mode)) != 0:
            raise ConexError("Invalid mode.")

    def AddHermitianMatrixInequalityFromEntries(self, n, d, ptr, row, col, val, variables=None):
        """c - sum_i y_i A_i positive semidefinite of order n over R / C / H (d = 1, 2, 4) with sparse Hermitian A_i and c
        given by the entries of their lower triangles and never expanded (CONEX_HIP_AddHermitianConstraintFromEntries,
        an extra next to the reference's surface).  The lists are those of AddLinearMatrixInequalityFromEntries; val is
        (nnz, d) real planes, or a complex array for d = 2; the upper triangle is the conjugate, so diagonal entries are
        real.  As for NewLinearMatrixInequality, the dual variable is the real plane and ComputeErrors does not cover
        the constraint.  UpdateLinearOperator and UpdateAffineTerm fail on it.  Returns the constraint id."""
        pt = np.ascontiguousarray(np.asarray(ptr).ravel(), dtype=np.int32)
        rw = np.ascontiguousarray(np.asarray(row).ravel(), dtype=np.int32)
        cl = np.ascontiguousarray(np.asarray(col).ravel(), dtype=np.int32)
        vl = np.asarray(val)
        if np.iscomplexobj(vl):
            if int(d) != 2:
                raise ConexError("Invalid LMI")
            vl = np.stack([vl.real.ravel(), vl.imag.ravel()], axis=1)
        vl = _f64(np.asarray(vl, dtype=np.float64).reshape(len(rw), -1))
        v = None if variables is None else np.ascontiguousarray(np.asarray(variables).ravel(), dtype=np.int64)
        m = self.m if v is None else len(v)
        if (n < 1 or d not in (1, 2, 4) or vl.shape != (len(rw), int(d)) or len(pt) != m + 2 or len(rw) != len(cl)
                or pt[-1] > len(rw) or np.any(np.diff(pt) < 0)):
            raise ConexError("Invalid LMI")
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        cid = self._L.CONEX_HIP_AddHermitianConstraintFromEntries(
            self.a, int(n), int(d), ip(pt), ip(rw), ip(cl), capi.dp(vl), m,
            None if v is None else v.ctypes.data_as(C.POINTER(C.c_long)))
        if cid < 0:
            raise ConexError("Failed to add constraint.")
        c = np.zeros((int(n), int(n)))  # (the real plane, as the other Hermitian builders keep)
        cs = slice(pt[m], pt[m + 1])
        c[rw[cs], cl[cs]] = vl[cs, 0]
        c[cl[cs], rw[cs]] = vl[cs, 0]
        self.c.append(c)
        self.num_constraints += 1
        return cid

    def SetSparseFold(self, mode):
        """Whether sparse Hermitian matrix inequalities over C or H sum over the top block row of their real
        representations: 1 every one, 0 none (CONEX_HIP_SetSparseFold)."""
        if self._L.CONEX_HIP_SetSparseFold(self.a, int(mode)) != 0:
            raise ConexError("Invalid mode.")

    def AddFactoredHermitianMatrixInequality(self, F, rank_ptr, sigma, c, variables=None):
        """c - sum_i y_i A_i positive semidefinite over R / C / H with low-rank Hermitian A_i = sum_k sigma[k] f_k f_k^*,
        k in rank_ptr[i]:rank_ptr[i + 1], given by its factors and never expanded
        (CONEX_HIP_AddFactoredHermitianConstraint, an extra next to the reference's surface).  F is (d, n, R) real planes
        of the hyper-complex columns f_k, d in {1, 2, 4}; rank_ptr has one entry more than the constraint has variables
        (len(variables), or all when None); sigma R entries or None (all +1); c is (d, n, n): plane 0 symmetric, the
        others skew.  As for NewLinearMatrixInequality, the dual variable is the real plane and ComputeErrors does not
        cover the constraint.  Returns the constraint id."""
        c = np.asarray(c, dtype=np.float64)
        F = np.asarray(F, dtype=np.float64)
        if c.ndim != 3 or c.shape[1] != c.shape[2] or F.ndim != 3 or F.shape[:2] != c.shape[:2]:
            raise ConexError("Invalid LMI")
        d, n, R = F.shape
        rp = np.ascontiguousarray(np.asarray(rank_ptr).ravel(), dtype=np.int32)
        sg = np.ones(R) if sigma is None else _f64(np.asarray(sigma, dtype=np.float64).ravel())
        if len(rp) < 1 or len(sg) != R:
            raise ConexError("Invalid LMI")
        v = None if variables is None else np.ascontiguousarray(np.asarray(variables).ravel(), dtype=np.int64)
        if len(rp) - 1 != (self.m if v is None else len(v)):
            raise ConexError("Invalid LMI")
        Ff = np.ascontiguousarray(np.swapaxes(F, -1, -2)).ravel()
        cf = np.ascontiguousarray(np.swapaxes(c, -1, -2)).ravel()
        cid = self._L.CONEX_HIP_AddFactoredHermitianConstraint(
            self.a, n, d, capi.dp(Ff), R, capi.dp(sg), rp.ctypes.data_as(C.POINTER(C.c_int)), len(rp) - 1, capi.dp(cf),
            None if v is None else v.ctypes.data_as(C.POINTER(C.c_long)))
        if cid < 0:
            raise ConexError("Failed to add constraint.")
        self.c.append(c[0].copy())
        self.num_constraints += 1
        return cid

    def AddQuadraticConstraint(self, Q, A, c, variables=None):
        """c - A y in {(x0, x1): x0 >= sqrt(x1' Q x1)}: the reference's QuadraticConstraint(Q, A, c), which it reaches
        through its C++ API only (an extra next to its Python surface, like CONEX_HIP_AddQuadraticConstraint itself).
        Q is n x n or None (the identity), A (n + 1) x len(variables) (x all variables when None), c has n + 1
        entries.  Returns the constraint id."""
        A = np.asarray(A, dtype=np.float64)
        c = _f64(np.asarray(c, dtype=np.float64).ravel())
        if A.ndim != 2 or A.shape[0] < 2 or len(c) != A.shape[0]:
            raise ConexError("Invalid quadratic constraint.")
        n = A.shape[0] - 1
        Af = capi.colmajor(A)
        Qf = None
        if Q is not None:
            Q = np.asarray(Q, dtype=np.float64)
            if Q.shape != (n, n):
                raise ConexError("Invalid quadratic constraint.")
            Qf = capi.colmajor(Q)
        v = None if variables is None else np.ascontiguousarray(np.asarray(variables).ravel(), dtype=np.int64)
        cid = self._L.CONEX_HIP_AddQuadraticConstraint(
            self.a, None if Qf is None else capi.dp(Qf), n, capi.dp(Af), n + 1, A.shape[1], capi.dp(c), n + 1,
            None if v is None else v.ctypes.data_as(C.POINTER(C.c_long)), 0 if v is None else len(v))
        if cid < 0:
            raise ConexError("Failed to add constraint.")
        self.num_constraints += 1
        return cid

    def AddStructuredQuadraticConstraint(self, S, F, sigma, A, c, variables=None):
        """The cone of AddQuadraticConstraint with Q = S + F diag(sigma) F' given by its parts and never formed
        (CONEX_HIP_AddStructuredQuadraticConstraint).  S is None, a triple (indptr, indices, data) or any object with
        those three attributes (a scipy CSR matrix), n x n with both triangles stored; F is None or (n, r); sigma None
        (all +1) or (r,).  Not both S and F None.  Returns the constraint id."""
        from .kkt import structured_q_parts
        A = np.asarray(A, dtype=np.float64)
        c = _f64(np.asarray(c, dtype=np.float64).ravel())
        if A.ndim != 2 or A.shape[0] < 2 or len(c) != A.shape[0]:
            raise ConexError("Invalid quadratic constraint.")
        n = A.shape[0] - 1
        try:
            rp, cl, vl = structured_q_parts(S, n)
        except ValueError as e:
            raise ConexError("Invalid quadratic constraint: %s" % e) from None
        rank, Ff, sg = 0, None, None
        if F is not None:
            F = np.asarray(F, dtype=np.float64)
            if F.ndim != 2 or F.shape[0] != n:
                raise ConexError("Invalid quadratic constraint.")
            rank = F.shape[1]
            Ff = capi.colmajor(F)
        if sigma is not None:
            sg = _f64(np.asarray(sigma, dtype=np.float64).ravel())
            if len(sg) != rank:
                raise ConexError("Invalid quadratic constraint.")
        if rp is None and rank == 0:
            raise ConexError("Invalid quadratic constraint: neither a sparse part nor factors.")
        Af = capi.colmajor(A)
        v = None if variables is None else np.ascontiguousarray(np.asarray(variables).ravel(), dtype=np.int64)
        ip = C.POINTER(C.c_int)
        cid = self._L.CONEX_HIP_AddStructuredQuadraticConstraint(
            self.a, n, None if rp is None else rp.ctypes.data_as(ip), None if rp is None else cl.ctypes.data_as(ip),
            None if rp is None else capi.dp(vl), rank, None if rank == 0 else capi.dp(Ff), None if sg is None else capi.dp(sg),
            capi.dp(Af), n + 1, A.shape[1], capi.dp(c), n + 1,
            None if v is None else v.ctypes.data_as(C.POINTER(C.c_long)), 0 if v is None else len(v))
        if cid < 0:
            raise ConexError("Failed to add constraint.")
        self.num_constraints += 1
        return cid

    def AddSparseQuadraticConstraint(self, Q, A, c, variables=None):
        """The cone of AddQuadraticConstraint / AddStructuredQuadraticConstraint with its (n + 1) x m matrix A given by
        its nonzeros and never formed (CONEX_HIP_AddSparseQuadraticConstraint).  A is a triple (indptr, indices, data)
        or any object with those three attributes (a scipy CSR matrix); row 0 is A0, the columns of a row may come in
        any order, explicit zeros are dropped; it has as many columns as `variables` has entries (every variable
        without).  Q is None (the identity), an (n, n) array, or the parts in the forms AddStructuredQuadraticConstraint
        takes, as a dict(S=, F=, sigma=) or a tuple (S, F, sigma).  Returns the constraint id."""
        from .kkt import csr_triple, quadratic_q_forms
        c = _f64(np.asarray(c, dtype=np.float64).ravel())
        n = len(c) - 1
        if n < 1:
            raise ConexError("Invalid quadratic constraint.")
        try:
            rp, cl, vl = csr_triple(A, n + 1, "A")
            dense, (qp, qc, qv), rank, Ff, sg = quadratic_q_forms(Q, n, "AddSparseQuadraticConstraint")
        except ValueError as e:
            raise ConexError("Invalid quadratic constraint: %s" % e) from None
        v = None if variables is None else np.ascontiguousarray(np.asarray(variables).ravel(), dtype=np.int64)
        m = self.m if v is None else len(v)
        ip = C.POINTER(C.c_int)
        cid = self._L.CONEX_HIP_AddSparseQuadraticConstraint(
            self.a, n, None if dense is None else capi.dp(dense), None if qp is None else qp.ctypes.data_as(ip),
            None if qp is None else qc.ctypes.data_as(ip), None if qp is None else capi.dp(qv), rank,
            None if rank == 0 else capi.dp(Ff), None if sg is None else capi.dp(sg),
            rp.ctypes.data_as(ip), cl.ctypes.data_as(ip), capi.dp(vl), n + 1, m, capi.dp(c), n + 1,
            None if v is None else v.ctypes.data_as(C.POINTER(C.c_long)), 0 if v is None else len(v))
        if cid < 0:
            raise ConexError("Failed to add constraint.")
        self.num_constraints += 1
        return cid

    # ---- entry-by-entry builders
    def _new(self, fn, *args, what="constraint"):
        cid = C.c_int()
        if fn(self.a, *args, C.byref(cid)) != 0:
            raise ConexError("Failed to add %s." % what)
        self.num_constraints += 1
        return cid.value

    def NewLinearMatrixInequality(self, order, hyper_complex_dim):
        cid = self._new(self._L.CONEX_NewLinearMatrixInequality, int(order), int(hyper_complex_dim))
        self.c.append(np.zeros((order, order)))
        return cid

    def NewLorentzConeConstraint(self, order):
        return self._new(self._L.CONEX_NewLorentzConeConstraint, int(order))

    def NewLinearInequality(self, num_rows):
        return self._new(self._L.CONEX_NewLinearInequality, int(num_rows))

    def NewQuadraticCost(self):
        return self._new(self._L.CONEX_NewQuadraticCost, what="quadratic cost")

    def UpdateQuadraticCostMatrix(self, cost_id, value, row, col):
        if self._L.CONEX_UpdateQuadraticCostMatrix(self.a, int(cost_id), float(value), int(row), int(col)) != 0:
            raise ConexError("Failed to update quadratic cost.")

    def UpdateLinearOperator(self, constraint, value, variable, row, col=0, hyper_complex_dim=0):
        if self._L.CONEX_UpdateLinearOperator(self.a, int(constraint), float(value), int(variable), int(row),
                                              int(col), int(hyper_complex_dim)) != 0:
            raise ConexError("Failed to update operator.")

    def UpdateAffineTerm(self, constraint, value, row, col=0, hyper_complex_dim=0):
        if self._L.CONEX_UpdateAffineTerm(self.a, int(constraint), float(value), int(row), int(col),
                                          int(hyper_complex_dim)) != 0:
            raise ConexError("Failed to update affine term.")

    # ---- solve
    def Maximize(self, b, config=None):
        cfg = config if config is not None else self.DefaultConfiguration()
        b = _f64(np.asarray(b, dtype=np.float64).ravel())
        if len(b) != self.m:
            raise ConexError("Cost vector dimension does not match number of variables.")
        sol = Solution()
        sol.y = np.ones(self.m)
        sol.status = self._L.CONEX_Maximize(self.a, capi.dp(b), len(b), C.byref(cfg), capi.dp(sol.y), len(sol.y))
        return sol

    def Solve(self, config=None):
        cfg = config if config is not None else self.DefaultConfiguration()
        cfg.enable_line_search = 1
        cfg.enable_rescaling = 0
        sol = Solution()
        sol.y = np.ones(self.m)
        sol.status = self._L.CONEX_Solve(self.a, C.byref(cfg), capi.dp(sol.y), len(sol.y))
        return sol

    def GetDualVariables(self):
        xs = []
        for i in range(self.num_constraints):
            rows = self._L.CONEX_GetDualVariableSize(self.a, i)
            shape = np.shape(self.c[i]) if i < len(self.c) else (rows,)
            if len(shape) == 2:
                buf = np.zeros(shape[0] * shape[1])
                self._L.CONEX_GetDualVariable(self.a, i, capi.dp(buf), shape[0], shape[1])
                xs.append(buf.reshape(shape[1], shape[0]).T.copy())
            else:
                buf = np.zeros(shape[0])
                self._L.CONEX_GetDualVariable(self.a, i, capi.dp(buf), shape[0], 1)
                xs.append(buf)
        return xs

    def ComputeErrors(self, y, xa, b):
        """Slacks s_i = c_i - A_i y and the optimality measures |b - sum_i A_i^* x_i|, <x, s>, the
        smallest eigenvalue (entry) of every s_i and x_i, for constraints added through Add*."""
        b = np.asarray(b, dtype=np.float64).ravel()
        err = Errors()
        slacks = []
        Ax = np.zeros(len(b))
        for op, c, x in zip(self.A, self.c, xa):
            s = np.asarray(c) - op.apply(y)
            slacks.append(s)
            Ax += op.adjoint(x)
            if s.ndim == 1:
                err.x_dot_s += float(s @ np.asarray(x).ravel())
                err.min_eig_S.append(float(s.min()))
                err.min_eig_X.append(float(np.asarray(x).min()))
            else:
                err.x_dot_s += float(np.trace(s @ x))
                err.min_eig_S.append(float(np.linalg.eigvalsh(0.5 * (s + s.T)).min()))
                err.min_eig_X.append(float(np.linalg.eigvalsh(0.5 * (x + np.asarray(x).T)).min()))
        err.Ax_minus_b = float(np.linalg.norm(b - Ax))
        return slacks, err
