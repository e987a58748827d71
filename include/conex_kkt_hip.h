/*
 * conex_kkt_hip.h -- C-ABI of the MI355X-native Newton-step KKT path.
 *
 * This is the "inner" drop-in boundary: the device-resident replacement for
 * what conex/cone_program.cc::Solve calls per IPM iteration.  The "outer"
 * boundary (the reference's interfaces/conex.h, 21 CONEX_* functions) is in
 * include/conex.h and is implemented on top of these entry points.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types cross the boundary
 *   - all matrices column-major fp64, all indices 32-bit int (as the reference)
 *   - every function returns 0 on success (CONEX_SUCCESS polarity,
 *     conex/error_codes.h) unless documented otherwise; no exception escapes
 *   - a context is bound to ONE HIP device and ONE stream and is not re-entrant
 *     (the reference's Program is not thread-safe either: kkt_solver.h:58,62)
 *   - host arrays are copied at call time (interfaces/conex.cc:143-159)
 *
 * Each entry point cites the reference interface it replaces.
 */
#ifndef CONEX_KKT_HIP_H
#define CONEX_KKT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cxk_context cxk_context;

enum { CXK_SUCCESS = 0, CXK_FAILURE = 1 };

/* cone types; the plugin surface of conex/constraint.h:51-197 */
enum {
  CXK_LMI = 0,    /* DenseLMIConstraint  dense_lmi_constraint.h:24-41 */
  CXK_LINEAR = 1, /* LinearConstraint    linear_constraint.h:14-84 */
  CXK_SOC = 2,    /* SOCConstraint       soc_constraint.h:6-54 */
  CXK_STATIC = 3, /* constant Schur block: QuadraticFunction quadratic_cost.cc:18-69,
                     SupernodalAssemblerStatic supernodal_assembler.h:122-129 */
  CXK_QUAD = 4,   /* QuadraticConstraint quadratic_cone_constraint.h:11-86: Lorentz cone
                     x0 >= sqrt(x1' Q x1) with an inner-product matrix Q on the vector part */
  CXK_OCT = 5     /* HermitianPsdConstraint<Octonions> hermitian_psd.cc:116-168, 171-230: Hermitian
                     matrices of order <= 3 over the octonions (cxk_add_hermitian with d = 8) */
};

/* ---- lifetime --------------------------------------------------------- */
/* Program(int number_of_variables) cone_program.h:101-104.
 * device < 0: host-only context (symbolic analysis works, numeric calls fail loudly).
 * stream: a hipStream_t (NULL = the device's null stream). */
int cxk_create(int num_vars, int device, void* stream, cxk_context** out);
void cxk_destroy(cxk_context* ctx);
const char* cxk_last_error(const cxk_context* ctx);

/* ---- constraint plugins: Program::AddConstraint(T, variables) cone_program.h:192-218,
 *      ConstraintManager::AddConstraint constraint_manager.h:50-64 (IsUnique check).
 *      Return the constraint id (>= 0) or -1 when rejected. vars == NULL means 0..num_vars-1. */
int cxk_add_lmi(cxk_context* ctx, int n, int m, const double* A /* m x (n x n) */,
                const double* C /* n x n */, const int* vars);
/* HermitianPsdConstraint<Real|Complex|Quaternions>(n, a, c) (hermitian_psd.h:41-52; what
 * CONEX_NewLinearMatrixInequality creates, interfaces/conex.cc:286-318).  d = 1, 2 or 4 real
 * planes; A = m x d planes of n x n (column-major, plane 0 symmetric, the others skew),
 * C = d planes.  W / dual variables are exchanged as d planes (cxk_dual_size = d n^2).  On the
 * device the cone is held through its real representation of order d n and runs on the LMI
 * kernels with the reference's Hermitian step rules (Taylor-squaring exponential, random-start
 * Lanczos, hermitian_psd.cc:10-91).  d = 8 (octonions, n <= 3): no real representation exists --
 * a cone type of its own (CXK_OCT) with the reference's octonion rules (hermitian_psd.cc:108-168:
 * quadratic representations in place of W A W, its heuristic step norms, GeodesicUpdateScaled). */
int cxk_add_hermitian(cxk_context* ctx, int n, int d, int m, const double* A, const double* C,
                      const int* vars);
/* Program::AddConstraint(EqualityConstraints{A, b}, vars) -> ConstraintManager::
 * AddEqualityConstraint (constraint_manager.h:66-90, equality_constraint.{h,cc}): A y[vars] = b,
 * A rows x m column-major.  Appends `rows` multipliers to the KKT system (cxk_system_size grows);
 * the Schur block is the constant [0 A^T; A 0] with AQc = [0; b].  Any equality switches
 * cxk_factor / the solves to the LDLT path (BlockLDLTInPlace block_triangular_operations.cc:
 * 315-349 over Eigen::RLDLT, RLDLT.h:298-431; kkt_solver.cc:180-193): factor always reports ok,
 * cxk_factor_regularized tells whether a pivot was clamped to +-1e-9.  cxk_get_W returns the
 * multipliers latched by the last cxk_prepare_step (lambda_, equality_constraint.cc:32-37). */
int cxk_add_equality(cxk_context* ctx, int rows, int m, const double* A /* rows x m */,
                     const double* b /* rows */, const int* vars);
int cxk_factor_regularized(cxk_context* ctx, int* flag);
int cxk_add_linear(cxk_context* ctx, int rows, int m, const double* A /* rows x m */,
                   const double* c /* rows */, const int* vars);
int cxk_add_soc(cxk_context* ctx, int n, int m, const double* A /* (n+1) x m */,
                const double* c /* n+1 */, const int* vars);
int cxk_add_static(cxk_context* ctx, int m, const double* G /* m x m */, const int* vars);
/* QuadraticConstraint(Q, A, c): c - A y in { (x0, x1) : x0 >= sqrt(x1' Q x1) }.  Q: n x n column-major,
 * symmetric positive definite, or NULL for the identity (the reference's two-argument constructor) */
int cxk_add_quadratic(cxk_context* ctx, int n, int m, const double* Q /* n x n or NULL */,
                      const double* A /* (n+1) x m */, const double* c /* n+1 */, const int* vars);
int cxk_num_constraints(const cxk_context* ctx);

/* Multi-GPU sharding (no reference counterpart -- the reference is single
 * process).  Must precede cxk_finalize.  This context then assembles/updates only the
 * constraints it owns (round-robin over elimination subtrees) and exposes a contiguous
 * exchange slab that the caller sum-reduces across ranks (RCCL all-reduce). */
int cxk_set_shard(cxk_context* ctx, int rank, int world_size);

/* Chain-shaped elimination trees (every step updates the next one only: BASELINE config 3 as the
 * reference's tests arrange it -- clique k = {8k .. 8k+9}, 5000 strictly dependent steps).  What the
 * getters below report is always the reference's order, supernodes, separators and permutation
 * (bit-identical: tests/test_symbolic_parity.py).  The FACTORIZATION of such a tree runs in a
 * segment-parallel order: the chain is cut into P pieces, the variables that carry an update across
 * a cut are eliminated last (in the root), the pieces become independent subtrees swept side by side
 * (symbolic.h, SegmentChain).  Same matrix, another elimination order: every result -- direction,
 * residuals, scaling points -- is the reference's to rounding (<= 1e-10 against the oracle); only the
 * stored factor differs, which is why cxk_get_slab / cxk_set_slab refuse such a context.
 * segments: 0 = the reference's order, P >= 2 = that many pieces; default (no call): the environment's
 * CXK_CHAIN_SEGMENTS, else automatic for chains of 256 steps or more.  Before cxk_finalize. */
int cxk_set_chain_segments(cxk_context* ctx, int segments);
int cxk_chain_segments(const cxk_context* ctx);

/* Reference identity: ON by default -- the library computes what the reference as written computes.
 * cxk_set_reference_identity(ctx, 0) (before cxk_finalize; or CXK_REFERENCE_QUIRKS=0 in the
 * environment) opts into two corrections of the reference:
 *   (i)  a constraint's Schur block is scattered by variable position also on fill-in supernodes,
 *        where BindDiagonalBlock's unchecked direct_update test (supernodal_assembler.cc:72-91)
 *        puts it one row and column off (a defect on rare structures);
 *   (ii) the Lanczos Ritz values of PrepareStep / GetWeightedSlackEigenvalues
 *        (approximate_eigenvalues.cc:178-239) are clamped to Samuelson's bound on the spectrum of
 *        W S (a noise-dominated Lanczos run near convergence otherwise yields an eigenvalue far
 *        outside the spectrum and a needlessly small step).
 * With identity on, CONEX_Maximize reproduces the iteration count and mu sequence of the reference
 * algorithm (tests/test_gpu_solver.py::test_reference_identity_reproduces_the_oracle_trajectory). */
int cxk_set_reference_identity(cxk_context* ctx, int on);

/* Second-order cones larger than LDS.  cxk_finalize admits a second-order cone to the LDS kernels when
 * its (n + 1) x (m + 2) image, the four vectors of TakeStep and the m + 3 (n + 1) doubles of PrepareStep
 * each fit the 163 328 B of a workgroup, and refuses any other.  Before cxk_finalize, on = 1: such a cone
 * is not refused; it is held in HBM and run by the streamed kernels (kernels_soc_stream.hip.h: the O(len)
 * maps on one striding workgroup per cone, G = 2 WA^T WA on the batched fp64 MFMA GEMM).  Cones that pass
 * the three demands keep today's kernels and today's bits.  Every output, getter and setter of a
 * streamed cone is that of any second-order cone; sharding, cxk_prepare_take_step and the device-selected
 * barrier parameter take it as they take the others.
 * Default (no call): the environment's CXK_STREAMED_CONES, else 0 = refuse.
 * Two limits remain with the switch on, refused at cxk_finalize with a message naming them: (n + 1) m or
 * m m beyond the int range; and the quadratic cone (cxk_add_quadratic), which keeps its LDS limits.
 * cxk_count_streamed_cones: constraints this context owns that run on the streamed kernels (-1 before
 * cxk_finalize; 0 on a host-only context, which chooses no kernels). */
int cxk_set_streamed_cones(cxk_context* ctx, int on);
int cxk_count_streamed_cones(const cxk_context* ctx);

/* Large linear-inequality blocks.  The LDS route (linear_schur, linear_prepare, linear_line_search) gives a
 * block one workgroup; the tiled route (kernels_linear_tiled.hip.h) spreads it over the chip: columns and row
 * tiles of 256 rows on their own workgroups, G = (diag(w) A)^T (diag(w) A) on the batched fp64 MFMA GEMM.
 * Before cxk_finalize, mode = 1: every linear block takes the tiled route; 0: none does, and a block over more
 * than 4096 variables -- which the LDS route's line search cannot launch -- is refused at cxk_finalize;
 * -1 (the default without a call: the environment's CXK_TILED_LINEAR = 0 | 1, else this): a block takes the
 * tiled route when it has more than 4096 variables or rows x variables^2 reaches the measured threshold
 * (kTiledLinearMinWork; CXK_TILED_LINEAR_MIN_WORK moves it for comparison runs).  Blocks on the LDS route keep
 * their kernels and their bits.  Every output, getter and setter of a tiled block is that of any linear block.
 * Refused on the tiled route at cxk_finalize, by name: rows x variables or variables^2 beyond the int range; a
 * group of equal blocks with more than 2^31 columns or row tiles.
 * cxk_count_tiled_linear: constraints this context owns that run on the tiled route (-1 before cxk_finalize;
 * 0 on a host-only context, which chooses no kernels). */
int cxk_set_tiled_linear(cxk_context* ctx, int mode);
int cxk_count_tiled_linear(const cxk_context* ctx);

/* Linear-inequality blocks evaluated from their nonzeros.  The LDS and the tiled route multiply a block as a dense
 * rows x variables matrix; bounds lb <= y <= ub, or the polytopic rows of an LP, QP or MPC problem, are almost
 * empty.  The sparse route (kernels_linear_sparse.hip.h) holds a block on the device by rows and by columns (CSR
 * and CSC) and never uploads its dense matrix: the assembly costs about sum_r nnz_r^2 multiply-adds and one write of
 * the variables x variables square, the slack passes nnz multiply-adds.  No atomics, fixed summation orders: two runs
 * give the same bits, and the per-row slack, W after a step, norminfd, normsqrd and the eigenvalue query are the tiled
 * route's bit for bit.  G comes out exactly symmetric.  Every output, getter and setter is that of any linear block.
 * cxk_set_sparse_linear, before cxk_finalize: mode 1 every linear block takes the sparse route; 0 none does; -1 a
 * block does when kSparseLinearMinRatio x sum_r nnz_r^2 <= rows x variables^2, rows x variables^2 is at least
 * kSparseLinearMinWork and no column has more than kSparseLinearMaxColumn rows (cone_route.h: 7.8, 8 192 000, 2048,
 * measured; CXK_SPARSE_LINEAR_MIN_RATIO moves the ratio for comparison runs) and neither cxk_set_tiled_linear
 * nor CXK_TILED_LINEAR made an explicit choice, which is a request for the dense kernels.  Without a call: the
 * environment's CXK_SPARSE_LINEAR = 0 | 1, else 0.  A sparse block may have more than 4096 variables whatever the
 * tiled mode.  Refused on the sparse route at cxk_finalize, by name: variables^2 beyond the int range; a group of
 * equal-shaped blocks with more than 2^31 nonzeros, column chunks or row tiles.
 * cxk_count_sparse_linear: constraints this context owns on the sparse route (-1 before cxk_finalize; 0 on a
 * host-only context); cxk_count_tiled_linear does not count them.
 * cxk_add_linear_csr: the constraint of cxk_add_linear given by its nonzeros, rowptr[r] .. rowptr[r + 1] being row
 * r's entries of col / val.  Columns within a row come in any order (the library sorts them); explicit zeros are
 * dropped.  Returns -1 (cxk_last_error names the reason) for rowptr[0] != 0, a decreasing rowptr, a column outside
 * [0, m), a column named twice in a row, null pointers.  Such a block can only take the sparse route: cxk_finalize
 * refuses it by name when the mode in force is 0.  A block added by cxk_add_linear may take any of the three routes. */
int cxk_set_sparse_linear(cxk_context* ctx, int mode);
int cxk_count_sparse_linear(const cxk_context* ctx);
int cxk_add_linear_csr(cxk_context* ctx, int rows, int m, const int* rowptr /* rows + 1 */, const int* col,
                       const double* val, const double* c /* rows */, const int* vars);

/* Second-order cones evaluated from their nonzeros.  The LDS and the streamed route hold a cone as a dense
 * (n + 1) x variables matrix; the cones of ||A x - b|| <= t with a sparse A, of robust LP rows or of trajectory norms
 * are almost empty.  The sparse route (kernels_soc_sparse.hip.h) holds a cone on the device by rows and by columns
 * (CSR and CSC), never uploads its dense matrix and evaluates, with J = diag(-1, 1, .., 1), u = A' w,
 *   G = 4 u u' + 2 det(w) H,  AW = 2 u,  AQc = 2 (2 (w . c) u + det(w) h),  sc = (2 w . c, 2 (2 (w . c)^2 + det(w) z)),
 * where H = A' J A, h = A' J c and z = c' J c are formed once, on the device, at cxk_finalize: one assembly is nnz
 * multiply-adds, one read of H and one write of G, with no (n + 1) x variables work space, no GEMM and no square
 * root.  These are quad_schur's expressions in w itself (Q = NULL); they differ from the literal 2 WA' WA of the other
 * two routes by rounding only.  No atomics, fixed summation orders: two runs give the same bits, G
 * comes out exactly symmetric, and the slack, the eigenvalue query, normsqrd, norminfd, the w^{1/2} PrepareStep leaves
 * in W and W after a step are the streamed route's bit for bit (its step kernels are reused).  Every output, getter
 * and setter is that of any second-order cone; cxk_line_search keeps refusing second-order cones.
 * cxk_set_sparse_soc, before cxk_finalize: mode 1 every second-order cone takes the sparse route; 0 none does; -1 a
 * cone does when it can run nowhere else (added by cxk_add_soc_csr, or (n + 1) x variables beyond the int range), or
 * when kSparseSocMinRatio x nnz <= (n + 1) x variables and (n + 1) x variables^2 is at least kSparseSocMinWork
 * (cone_route.h, measured; CXK_SPARSE_SOC_MIN_RATIO moves the ratio for comparison runs).  Without a call: the
 * environment's CXK_SPARSE_SOC = 0 | 1, else 0.  A sparse cone needs neither cxk_set_streamed_cones nor LDS room.
 * Refused on the sparse route at cxk_finalize, by name: variables^2 beyond the int range; a group of equal-shaped
 * cones with more than 2^31 nonzeros, column chunks, row tiles or tiles of the Schur block.
 * cxk_count_sparse_soc: constraints this context owns on the sparse route (-1 before cxk_finalize; 0 on a host-only
 * context); cxk_count_streamed_cones does not count them.
 * cxk_sparse_soc_setup_ms: device milliseconds the last cxk_finalize spent forming H, h and z of this context's sparse
 * cones (hipEvent pair around those launches; 0 without such cones, before cxk_finalize and on a host-only context).
 * cxk_add_soc_csr: the constraint of cxk_add_soc given by the nonzeros of its (n + 1) x m matrix, rowptr[r] ..
 * rowptr[r + 1] being row r's entries of col / val.  Columns within a row come in any order (the library sorts them);
 * explicit zeros are dropped.  Returns -1 (cxk_last_error names the reason) for rowptr[0] != 0, a decreasing rowptr, a
 * column outside [0, m), a column named twice in a row, null pointers.  Such a cone has no dense matrix and can only
 * take the sparse route: cxk_finalize refuses it by name when the mode in force is 0.  A cone added by cxk_add_soc
 * takes the sparse route under mode 1 or when the automatic rule picks it (its nonzeros are read off A at
 * cxk_finalize) and keeps its present kernels and bits otherwise. */
int cxk_set_sparse_soc(cxk_context* ctx, int mode);
int cxk_count_sparse_soc(const cxk_context* ctx);
double cxk_sparse_soc_setup_ms(const cxk_context* ctx);
int cxk_add_soc_csr(cxk_context* ctx, int n, int m, const int* rowptr /* n + 2 */, const int* col, const double* val,
                    const double* c /* n + 1 */, const int* vars);

/* Matrix inequalities of any order (kernels_lmi_large.hip.h, kernels_lmi_wide.hip.h).  A real symmetric LMI beyond
 * order 1024 factors its Pade system with a panel kernel whose row count no workgroup bounds (lu_panel_tall; the
 * orders up to 1024 keep their kernel and bits).  The two-sided Lanczos run behind PrepareStep and the eigenvalue
 * query keeps its vectors in the LDS of one workgroup up to a real-representation order of 2549; the chip-wide run
 * keeps them in HBM and spreads every matrix pass over 64 x 64 tiles: the same recurrence, start vector, break rule
 * and outputs, other summation orders (fixed ones, no atomics: two runs give the same bits).
 * cxk_set_wide_spectrum, before cxk_finalize: mode -1 (the default) a large-order group (order above 60) takes the
 * chip-wide run only above order 2549, so that no shape that ran before changes its kernels or bits; 0 never: an order
 * above 2549 is then refused by cxk_finalize, by name; 1 every large-order group.  Without a call: the environment's
 * CXK_WIDE_SPECTRUM = -1 | 0 | 1.  cxk_finalize also refuses, by name, an order above 46340 (the kernels index the
 * n x n entries with ints).  The factored routes (cxk_add_lmi_factored, cxk_add_hermitian_factored) keep their limits
 * of 1024 and 2549.
 * cxk_count_wide_spectrum: constraints this context owns whose groups take the chip-wide run (-1 before cxk_finalize; 0
 * on a host-only context). */
int cxk_set_wide_spectrum(cxk_context* ctx, int mode);
int cxk_count_wide_spectrum(const cxk_context* ctx);

/* Matrix inequalities given by their nonzeros (kernels_lmi_sparse.hip.h).  cxk_add_lmi_coo adds the constraint of
 * cxk_add_lmi (DenseLMIConstraint semantics, real symmetric): list i < m, ptr[i] .. ptr[i + 1], holds the entries of
 * A_i, list m those of C, as (row, col, val) with row >= col: the caller gives the lower triangle and the library
 * mirrors it, so the data is symmetric by construction.  Entries of a list come in any order, explicit zeros are
 * dropped, an empty list is the zero matrix.  Each mirrored list is sorted by column, then row -- the order in which a
 * dense matrix given to cxk_add_lmi is scanned -- so the same data gives the same device lists and the same bits as
 * cxk_add_lmi on the sparse route.  The record keeps the lists and the n x n square of C (the size of W); nothing of
 * size m n^2 is allocated on the host or the device.  Returns -1 (cxk_last_error names the reason, prefixed
 * "cxk_add_lmi_coo: ") for n < 1, m < 0, null pointers, ptr[0] != 0, a decreasing ptr, an index outside [0, n),
 * row < col, a position named twice in a list, a value that is not finite, and n or m above 32767 (the entry table
 * packs row | col << 16 and the pair table i | j << 16 into ints that the kernels unpack with signed shifts).  Such a
 * constraint can only take the sparse route (cxk_count_sparse_lmi counts it) whatever LmiSparsePays says: with
 * CXK_SPARSE_LMI=0 in force cxk_finalize refuses it by name.  Every getter, setter and output is that of an LMI.
 * The affine term of a sparse LMI beyond the LDS-resident orders (order 64 and up) with more than 64 nonzeros is by
 * default multiplied out, X = W C W, by two n^3 GEMMs.  cxk_set_sparse_affine, before cxk_finalize: mode 1 every such
 * group instead forms (W C)' from C's nonzeros (n nnz(C) multiply-adds) and X only at the positions that an entry of
 * some A_i or of C names (n multiply-adds each), then AQc, <c,Qc> and <w,c> from those; 0 none does (the GEMMs: the
 * bits of before); -1 a constraint does when LmiSparseAffinePays(n, nnz(C), positions) (cone_route.h, measured).
 * Without a call: the environment's CXK_SPARSE_AFFINE = -1 | 0 | 1, else 0 for a constraint added by cxk_add_lmi or
 * cxk_add_hermitian (nothing that ran before changes its kernels or bits) and -1 for one added by cxk_add_lmi_coo.
 * Constraints that differ in the outcome do not share a group.  Fixed summation orders, no atomics: two runs give the
 * same bits; the values differ from the GEMM path's by rounding only.
 * cxk_count_sparse_affine: constraints this context owns on those kernels (-1 before cxk_finalize; 0 on a host-only
 * context); cxk_lmi_kernels reports "lmi_schur_sparse hbm sparse-C" for them. */
int cxk_add_lmi_coo(cxk_context* ctx, int n, int m, const int* ptr /* m + 2 */, const int* row, const int* col,
                    const double* val, const int* vars);
int cxk_set_sparse_affine(cxk_context* ctx, int mode);
int cxk_count_sparse_affine(const cxk_context* ctx);

/* Hermitian matrix inequalities over R / C / H given by their nonzeros.  cxk_add_hermitian_coo adds the constraint of
 * cxk_add_hermitian(ctx, n, d, m, A, C, vars), d in {1, 2, 4}, by entries: the lists work as for cxk_add_lmi_coo (list
 * i < m is A_i, list m is C, row >= col, any order within a list, an empty list is the zero matrix); the value of entry
 * s is the d planes val[d s .. d s + d - 1] (for d = 2 the memory of a complex double).  The library mirrors with the
 * conjugate: X_0[c,r] = X_0[r,c], X_p[c,r] = -X_p[r,c] for p >= 1.  An entry whose planes are all zero is dropped, and
 * a zero plane of a kept entry makes no real entry.  The record is that of cxk_add_hermitian (herm_d = d, order
 * N = d n) without the dense matrices: its lists hold the nonzeros of the real representations, built directly --
 * block (k, j) of L(X) is sign[k ^ j][j] X_{k ^ j} (the reference's sign table), at row k n + r, column j n + c --
 * each sorted by column then row, exactly the lists that the sparse route reads off the dense matrices of
 * cxk_add_hermitian; and the N x N square of L(C).  Nothing of size m N^2 is allocated on the host or the device.
 * Getters and setters speak d planes, as for every Hermitian constraint.  Returns -1 (cxk_last_error names the reason,
 * prefixed "cxk_add_hermitian_coo: ") for n < 1, m < 0, a d that is not 1, 2 or 4 (8: the octonions have no real
 * representation), null pointers, ptr[0] != 0, a decreasing ptr, an index outside [0, n), row < col, a position named
 * twice in a list, a plane that is not finite, a diagonal entry with a nonzero plane p >= 1, and d n or m above 32767.
 * Such a constraint can only take the sparse route: with CXK_SPARSE_LMI=0 in force cxk_finalize refuses it by name.
 * The folded sums (kernels_lmi_sparse.hip.h): for a real representation M, tr M / d is the trace of its top-left
 * n x n block, so tr(L(A_i) W L(A_j) W) / d, tr(L(A_i) W) / d and tr(L(A_i) W C W) / d need only the entries of L(A_i)
 * in its top block row, 1 / d of them: a folded group runs every sum over a first list over those and multiplies by no
 * 1 / d.  cxk_set_sparse_fold, before cxk_finalize: mode 1 every sparse Hermitian group with d > 1 folds, 0 none does
 * (the bits of before).  Without a call: the environment's CXK_SPARSE_FOLD = 0 | 1, else 0 for a constraint added by
 * cxk_add_hermitian (nothing that ran before changes its kernels or bits) and 1 for one added by
 * cxk_add_hermitian_coo.  d = 1 never folds.  Constraints that differ in the outcome do not share a group.  Fixed
 * summation orders, no atomics: two runs give the same bits; the values differ from the unfolded ones by rounding.
 * cxk_count_sparse_fold: constraints this context owns on the folded kernels (-1 before cxk_finalize; 0 on a host-only
 * context); cxk_lmi_kernels reports the name of the sparse instance with the suffix " folded" for them. */
int cxk_add_hermitian_coo(cxk_context* ctx, int n, int d, int m, const int* ptr /* m + 2 */, const int* row,
                          const int* col, const double* val /* d per entry */, const int* vars);
int cxk_set_sparse_fold(cxk_context* ctx, int mode);
int cxk_count_sparse_fold(const cxk_context* ctx);

/* Low-rank matrix inequalities given by their factors (kernels_lmi_factored.hip.h).  cxk_add_lmi_factored adds the
 * constraint of cxk_add_lmi (DenseLMIConstraint semantics, real symmetric) with
 *   A_i = sum_k sigma_k f_k f_k',  k = rank_ptr[i] .. rank_ptr[i + 1] - 1,
 * f_k the columns of F (n x R, column-major, R = rank_ptr[m]); sigma = NULL means all +1; rank_ptr[i + 1] == rank_ptr[i]
 * makes A_i the zero matrix.  The A_i are never formed, on the host or on the device: with Z = W F, P = F' Z, Y = C Z
 * (three products on the fp64 MFMA GEMM) G(i,j) = sum sigma_k sigma_l P_kl^2, AW(i) = sum sigma_k P_kk,
 * AQc(i) = sum sigma_k z_k' y_k, and the slack is F diag(sigma_k y_i(k)) F' - kC; O(n^2 R + n R^2) work per assembly
 * instead of O(n^3 m + n^2 m^2).  Behind the slack the constraint runs the large-order LMI route unchanged, whatever
 * its order, and every getter, setter and output is that of an LMI (cxk_set_W, cxk_get_W, cxk_dual_size, ..).  Fixed
 * summation orders, no atomics: two runs give the same bits.  Constraints of equal n, m and R share launches; their
 * rank_ptr and sigma may differ.
 * Returns the constraint id, or -1 (cxk_last_error names the reason) for: n < 1, m < 0; null rank_ptr, C or (R > 0) F;
 * rank_ptr[0] != 0; a decreasing rank_ptr; a value of F, sigma or C that is not finite; a C that is not symmetric.
 * Refused at cxk_finalize, by name: n > 1024 (the Pade LU of the large-order TakeStep); n R, R R or m m beyond the
 * int range; more than 65535 such constraints of one shape.
 * A context holding such a constraint reports cxk_device_mu_supported == 0 and cxk_triple_supported == 0, keeps its
 * assembly and its tree in separate launches, and cxk_line_search refuses it as it refuses every non-linear cone.
 * The route is not one of the LMI kernel instances: cxk_lmi_kernels fails for such a constraint and
 * cxk_count_lmi_kernel does not count it.  cxk_assembly_work counts the route's own flops and bytes.
 * cxk_count_factored_lmi: constraints this context owns on this route (-1 before cxk_finalize; a host-only context
 * counts them too: the route is how they were added, not a choice of cxk_finalize). */
int cxk_add_lmi_factored(cxk_context* ctx, int n, int m, const int* rank_ptr /* m + 1 */, const double* F /* n x R */,
                         const double* sigma /* R, NULL = all +1 */, const double* C /* n x n */, const int* vars);
int cxk_count_factored_lmi(const cxk_context* ctx);

/* Low-rank Hermitian matrix inequalities over R / C / H given by their factors: cxk_add_hermitian_factored adds the
 * constraint of cxk_add_hermitian(ctx, n, d, m, A, C, vars), d in {1, 2, 4}, with
 *   A_i = sum_k sigma_k f_k f_k^*,  k = rank_ptr[i] .. rank_ptr[i + 1] - 1,
 * f_k the hyper-complex columns of F (d planes of n x R, column-major, R = rank_ptr[m]); C is d planes of n x n as
 * cxk_add_hermitian takes them.  Neither the A_i nor their real representations L(A_i) are formed.  The record is
 * Hermitian (cxk_get_W / cxk_set_W / cxk_dual_size speak d planes) and factored (everything said of
 * cxk_add_lmi_factored's constraint above holds, cxk_count_factored_lmi counts it).  With N = d n the device holds
 * L(F) (N x dR: d times F; its first R columns F0 are the stacked planes), sigma, the pointers and L(C).  Only F0
 * passes through W and C: Z = W F0, Y = C Z (N x R), P = L(F)' Z (d planes of R x R in one product), then
 * G(i,j) = sum sigma_k sigma_l sum_p P_p(k,l)^2, AW(i) = sum sigma_k P_0(k,k), AQc(i) = sum sigma_k z_k' y_k, every
 * contraction being tr / d as for cxk_add_hermitian; the slack is L(F) diag(sigma_k y_i(k)) L(F)' - k L(C): its first
 * n columns from one N x n x dR product, the other block columns filled from them, so that it is exactly a real
 * representation.  The assembly first replaces W by the real representation nearest to it (TakeStep leaves it one
 * only to rounding, and the folded sums read W through one column block of L(F)); a W that is one keeps its bits.
 * Behind the slack run the large-order route's Hermitian rules (Taylor-squaring exponential, random-start Lanczos).  Fixed summation orders, no atomics: two runs give the same bits.
 * Returns the constraint id, or -1 (cxk_last_error names the reason, prefixed "cxk_add_hermitian_factored: ") for:
 * n < 1, m < 0; d not 1, 2 or 4 (the octonions, d = 8, have no real representation); null rank_ptr, C or (R > 0) F;
 * rank_ptr[0] != 0; a decreasing rank_ptr; a value of F, sigma or C that is not finite; a C that is not Hermitian
 * (plane 0 symmetric, the others skew).
 * Refused at cxk_finalize, by name: N R, d R R, N dR or m m beyond the int range; an order N above 2549, whose Lanczos
 * vectors (lmi_large_spectrum) exceed LDS -- the Taylor TakeStep has no LU, so cxk_add_lmi_factored's limit of 1024
 * does not apply. */
int cxk_add_hermitian_factored(cxk_context* ctx, int n, int d, int m, const int* rank_ptr /* m + 1 */,
                               const double* F /* d planes of n x R, column-major */, const double* sigma /* R or NULL */,
                               const double* C /* d planes of n x n, as cxk_add_hermitian */, const int* vars);

/* Quadratic cones { x0 >= sqrt(x1' Q x1) } of real size.  The LDS route (quad_schur, quad_prepare, quad_take_step)
 * gives a cone one workgroup and runs its maps, the products with Q among them, on one thread; a cone whose
 * variables + 4 (dimension + 1) doubles exceed LDS is refused at cxk_finalize.  The streamed route
 * (kernels_quad_stream.hip.h) keeps the cone and Q in HBM: the products with Q on a grid of row tiles and column
 * splits (up to two vectors per pass over Q; one pass per assembly, two per PrepareStep or eigenvalue query, none
 * per TakeStep), the O(n) maps on one 256-thread workgroup per cone, A1' Q A1 on the batched fp64 MFMA GEMM at
 * cxk_finalize.  No atomics, fixed summation orders: two runs give the same bits (not the LDS route's bits).
 * Before cxk_finalize, mode = 1: every quadratic cone takes the streamed route; 0 (the default without a call: the
 * environment's CXK_STREAMED_QUADRATIC = 0 | 1, else 0): none does, and the refusal above stands, whatever
 * cxk_set_streamed_cones says; -1: a cone takes it when it fails one of the LDS route's three demands or when the
 * doubles streamed per pass, (Q ? n n : 0) + (n + 1) m, reach the measured threshold (kQuadStreamMinWork;
 * CXK_STREAMED_QUADRATIC_MIN_WORK moves it for comparison runs).  Cones on the LDS route keep their kernels and
 * their bits.  Every output, getter and setter of a streamed cone is that of any quadratic cone.
 * A cone added by cxk_add_quadratic_structured or cxk_add_quadratic_csr (below) has no LDS form: it takes the streamed
 * route under every mode, 0 included.
 * Refused on the streamed route at cxk_finalize, by name: (dimension + 1) x variables, variables^2 or the entries
 * of Q beyond the int range; a group of equal cones with more than 2^31 columns, row tiles or blocks.
 * cxk_count_streamed_quadratic: constraints this context owns that run on the streamed route (-1 before
 * cxk_finalize; 0 on a host-only context, which chooses no kernels); cxk_count_streamed_cones keeps counting
 * second-order cones only. */
int cxk_set_streamed_quadratic(cxk_context* ctx, int mode);
int cxk_count_streamed_quadratic(const cxk_context* ctx);

/* The quadratic cone of cxk_add_quadratic with Q = S + F diag(sigma) F' given by its parts and never formed: factor-model
 * risk (D + F Sigma F'), generalised least squares with a banded or graph-structured precision matrix, energy bounds
 * with a stiffness matrix, Q = L L' known by its factor.
 *   S      n x n by its nonzeros in CSR (q_rowptr: n + 1 ints from 0, q_col, q_val), multiplied as given: BOTH triangles
 *          are stored; symmetry and definiteness of Q are the caller's duty, as with the dense Q.  Duplicate entries of a
 *          row are summed (in the order they are stored when one lane works on a row).  q_rowptr = NULL: no sparse part.
 *   F      n x rank column-major, sigma rank entries of either sign (NULL: all +1).  rank = 0: no factors.
 * Refused by name (cxk_last_error): q_rowptr[0] != 0 or decreasing, a column outside [0, n), a value of q_val, F or
 * sigma that is not finite, rank < 0, and both parts absent (for the identity pass Q = NULL to cxk_add_quadratic).
 * The constraint keeps the CSR arrays, F and sigma; nothing of n x n is allocated on the host or the device at any
 * point, and the streamed route's refusal of an order beyond 46 340 (n^2 past the int range) does not apply; the demands
 * on (n + 1) m and m^2 stay, and the nonzeros of a group of equal cones must fit an int.  A host-only context takes the
 * call; the problem's structure (cliques, fill, order) is that of cxk_add_quadratic with the same A and vars.
 * Such a cone always runs on the streamed kernels (kernels_quad_structured.hip.h makes the products with Q: the factor
 * dots on cone x factor x row segment workgroups, then one kernel over row tiles with 1, 8 or 64 lanes per row of S by
 * the mean nonzeros per row -- CXK_QUAD_CSR_LANES = 1 | 8 | 64 overrides); it has no LDS form, so
 * cxk_set_streamed_quadratic(ctx, 0) does NOT refuse it and it counts in cxk_count_streamed_quadratic whatever the
 * mode.  Cones of equal (n, m, rank, with or without S) share a group even when their nonzero counts differ.  Every
 * output, getter and setter is that of any quadratic cone.  No atomics, fixed summation orders: same bits every run.
 * cxk_count_structured_quadratic: constraints this context owns that were added this way (-1 before cxk_finalize; 0 on
 * a host-only context, which chooses no kernels). */
int cxk_add_quadratic_structured(cxk_context* ctx, int n, int m,
                                 const int* q_rowptr /* n + 1, or NULL: no sparse part */, const int* q_col, const double* q_val,
                                 int rank, const double* F /* n x rank column-major, or NULL when rank = 0 */,
                                 const double* sigma /* rank, NULL = all +1 */,
                                 const double* A /* (n+1) x m */, const double* c /* n+1 */, const int* vars);
int cxk_count_structured_quadratic(const cxk_context* ctx);

/* The quadratic cone of cxk_add_quadratic or cxk_add_quadratic_structured with its (n + 1) x m matrix A given by its
 * nonzeros and never formed: a risk bound over assets (A1 = [I 0], A0 = e_t), a generalised-least-squares residual
 * that touches a few variables per row.
 *   A      (n + 1) x m in CSR (a_rowptr: n + 2 ints from 0, a_col, a_val); row 0 is A0.  The columns of a row may
 *          come in any order (the library sorts them); explicit zeros are dropped.
 *   Q      n x n dense column-major, OR its parts as cxk_add_quadratic_structured takes them, OR neither (Q = NULL,
 *          q_rowptr = NULL, rank = 0, F = NULL, sigma = NULL): the identity.
 * Refused by name (cxk_last_error): a_rowptr[0] != 0 or decreasing, a column outside [0, m), a column named twice in
 * a row, a value of a_val, c or Q that is not finite, a_rowptr or c null, Q given dense and by its parts, and every
 * refusal cxk_add_quadratic_structured makes for the parts.
 * The constraint keeps the nonzeros only: nothing of (n + 1) x m or n x m is allocated on the host or on the device
 * at any point, cxk_finalize included, and the streamed route's refusal of (n + 1) x m beyond the int range does not
 * apply; m^2, a dense Q's n^2 and the nonzeros of a group of equal cones must fit an int.  A host-only context takes
 * the call; the problem's structure (cliques, fill, order) and every getter are those of cxk_add_quadratic with the
 * same vars.
 * Such a cone always runs on the streamed kernels, as a structured one does, under every mode of
 * cxk_set_streamed_quadratic, 0 included, with the four places that read A replaced (kernels_quad_sparse.hip.h):
 * v = A'(W0, Q w1) by one wavefront per column through the CSC (u = A1' Q c1 is constant and made once at
 * cxk_finalize), row 0 from a dense copy of it, the slack by the sparse second-order cones' kernel, and
 * A_gram = A1' Q A1 at cxk_finalize in panels of a few columns (work space 2 n P doubles per cone).  Cones of equal
 * (n, m, form of Q, rank) share a group whatever their patterns.  No atomics, fixed summation orders: same bits every
 * run, and the bits of ascending input whatever the order of the columns given.
 * cxk_count_sparse_quadratic: constraints this context owns that were added this way (-1 before cxk_finalize; 0 on a
 * host-only context, which chooses no kernels); they count in cxk_count_streamed_quadratic too, and in
 * cxk_count_structured_quadratic when Q came by its parts. */
int cxk_add_quadratic_csr(cxk_context* ctx, int n, int m,
                          const double* Q /* n x n dense, or NULL */,
                          const int* q_rowptr, const int* q_col, const double* q_val,
                          int rank, const double* F, const double* sigma /* as cxk_add_quadratic_structured; all absent = none */,
                          const int* a_rowptr /* n + 2 */, const int* a_col, const double* a_val,
                          const double* c /* n + 1 */, const int* vars);
int cxk_count_sparse_quadratic(const cxk_context* ctx);

/* Initialize(): symbolic analysis (SupernodalKKTSolver ctor kkt_solver.cc:104-116),
 * Bind (kkt_solver.h:26-33), workspace carve + SetIdentity (cone_program.cc:78-112),
 * upload of constant data, construction of device index tables and level schedule.
 * Environment read here: CXK_SPARSE_LMI=0/1 (force the dense / sparse LMI evaluation),
 * CXK_REFERENCE_QUIRKS=0 (= cxk_set_reference_identity(ctx, 0) unless that was called). */
int cxk_finalize(cxk_context* ctx);

/* ---- symbolic results (MatrixData supernodal_solver.h:18-29; bit-exact vs reference) */
int cxk_system_size(const cxk_context* ctx); /* N */
int cxk_get_order(const cxk_context* ctx, int* order /* K */);
int cxk_get_permutation(const cxk_context* ctx, int* perm, int* perm_inv /* num_vars */);
/* which: 0 cliques(permuted) 1 supernodes_orig 2 separators_orig 3 supernodes_pos
 *        4 separators_pos ; returns length (out may be NULL) */
int cxk_get_list(const cxk_context* ctx, int which, int e, int* out);
int cxk_get_supernode_sizes(const cxk_context* ctx, int* out /* K */);
long cxk_slab_size(const cxk_context* ctx);
int cxk_get_block_offsets(const cxk_context* ctx, long* diag_off, long* offd_off /* K */);
int cxk_get_ss_index(const cxk_context* ctx, int e, long* out); /* returns count */
int cxk_num_levels(const cxk_context* ctx);

/* ---- scaling point W (workspace()->W, constraint.h:159-167) ------------ */
int cxk_set_identity(cxk_context* ctx);                       /* SetIdentity */
int cxk_dual_size(const cxk_context* ctx, int i);
int cxk_get_W(cxk_context* ctx, int i, double* out);          /* get_dual_variable */
int cxk_set_W(cxk_context* ctx, int i, const double* in);     /* warm start import */

/* ---- Newton step, device resident ------------------------------------- */
/* solver->Assemble() + AssembleSchurComplementResiduals  cone_program.cc:338-341 */
int cxk_assemble(cxk_context* ctx);
/* solver->Factor() kkt_solver.cc:172-199 (LLT mode). *ok = 1 success, 0 not PD. Syncs. */
int cxk_factor(cxk_context* ctx, int* ok);
/* The same without waiting: cxk_factor_async enqueues the factorization, cxk_factor_status
 * returns its LLT flag -- at no cost when a later blocking call (cxk_prepare_step,
 * cxk_weighted_slack_eigenvalues, cxk_step_scalars, cxk_sync) has already waited for the stream:
 * every wait brings the flag, the reduced step info and the step scalars back together through
 * one pinned host mailbox.  conex::Solve's per-iteration host round trips (cone_program.cc:360,
 * 417, 439-446) collapse into one or two this way. */
int cxk_factor_async(cxk_context* ctx);
/* factor and, in the same sweeps, solve  y <- K^-1 (cb b + cq AQc + cw AW)  (permuted b, residuals of
 * the last cxk_assemble): one upward pass instead of factor + forward substitution.  (k bs, k cs, -2)
 * gives the Newton direction of cxk_newton_direction, (-bs, cs, 0) the solve of
 * ComputeMuFromDivergence (cone_program.cc:173-214).  LLT flag through cxk_factor_status. */
int cxk_factor_solve_async(cxk_context* ctx, double cb, double cq, double cw);
/* cxk_factor_async + cxk_newton_direction in one upward pass (same right-hand side formula
 * y = k (b bs + AQc cs) - 2 AW, cone_program.cc:409-411) */
int cxk_factor_direction_async(cxk_context* ctx, double k, double bs, double cs);
int cxk_factor_status(cxk_context* ctx, int* ok);
/* enqueue the by / cx / norm reductions of cxk_step_scalars; the next cxk_step_scalars call
 * returns them (waiting only if nothing has waited since) */
int cxk_step_scalars_async(cxk_context* ctx);
/* y_dev = inv_sqrt_mu*(b*b_scaling + AQc*c_scaling) - 2 AW  cone_program.cc:409-411,
 * followed by solver->SolveInPlace(&y) kkt_solver.cc:220-263.  No host sync. */
int cxk_set_cost(cxk_context* ctx, const double* b /* num_vars, host */);
int cxk_newton_direction(cxk_context* ctx, double inv_sqrt_mu, double b_scaling,
                         double c_scaling);
/* y_dev = cb*b + cq*AQc + cw*AW, then SolveInPlace: covers the Newton right-hand side
 * (k*bs, k*cs, -2), the mu-rule solve of ComputeMuFromDivergence cone_program.cc:181
 * (-bs, cs, 0) and the dual-recovery solve cone_program.cc:504 (k*bs, 0, -1).  No host sync. */
int cxk_solve_rhs(cxk_context* ctx, double cb, double cq, double cw);
/* the scalars of one IPM iteration (cone_program.cc:343-357, 439-446), computed on device:
 * out = { b.y, AQc.y, |b|^2, |AQc|^2, <w,c>, <c,Qc> }.  Syncs. */
int cxk_step_scalars(cxk_context* ctx, double* out6);
/* whole BASELINE metric unit: assemble + factor + rhs + solve, asynchronous on the stream;
 * factor status is latched and returned by cxk_sync. */
int cxk_kkt_solve_async(cxk_context* ctx, double inv_sqrt_mu, double b_scaling,
                        double c_scaling);
int cxk_sync(cxk_context* ctx, int* factor_ok);
/* Vectors in the ORIGINAL VARIABLE ORDER -- cxk_solve_inplace, cxk_get_y, cxk_set_y, cxk_get_residuals,
 * cxk_get_valid_variables -- are indexed by variable: entry v belongs to variable v, the multipliers of the equality
 * blocks follow the num_vars variables.  Their length, V below, is num_vars + multipliers.  V = N when every
 * variable occurs in some constraint.  A program that leaves variables out has a smaller N (cxk_system_size
 * counts the variables that occur) and the same indices: entries of unused variables are neither read nor written,
 * but the vector still has V entries, and a shorter one is read and written past its end. */
/* SolveInPlace on a host vector of length V (copy in, solve, copy out). */
int cxk_solve_inplace(cxk_context* ctx, double* y);
/* Y <- K^-1 Y for nrhs columns with the factor of the latest factorization.  Y is N x nrhs, column-major with
 * leading dimension ld >= N, in the ORIGINAL variable order (cxk_solve_inplace's convention; a program that leaves
 * out a variable below the largest one it uses is refused: N rows would not hold every index).  The plain factor
 * solve: level-scheduled block substitution, cxk_solve_block_chunk_width() columns per workgroup, the factor read
 * once per chunk; column j of the result depends on column j of the input only, runs are bit-reproducible.
 * Leaves y, W, the slab, the residuals and the three solutions of cxk_factor_solve_triple_async alone.  Refused
 * (cxk_last_error names the reason): no successful factorization yet, nrhs < 1, ld < N, a null pointer, a sharded
 * context, QR solver mode, cxk_set_iterative_refinement > 0.  Waits only where the outcome of the latest
 * factorization has not been read yet. */
int cxk_solve_block(cxk_context* ctx, double* Y_host, int ld, int nrhs);        /* copies in, solves, copies out, waits */
int cxk_solve_block_device(cxk_context* ctx, double* Y_dev, int ld, int nrhs);  /* device pointer, enqueued on the context's stream, does not wait */
int cxk_solve_block_chunk_width(void);
/* (sharded context with a communicator: a COLLECTIVE -- a sum all-reduce of N doubles assembles the
 * whole vector, so every rank must call it, in the same order relative to its other cxk_* calls) */
int cxk_get_y(cxk_context* ctx, double* y /* V, original variable order (above cxk_solve_inplace) */);
int cxk_set_y(cxk_context* ctx, const double* y /* V */);

/* PrepareStep over all constraints (cone_program.h:69-90); info = {normsqrd, norminfd}.
 * Uses the device-resident y.  Syncs (returns two scalars). */
int cxk_prepare_step(cxk_context* ctx, int affine, double c_weight, double e_weight,
                     double* info);
/* cxk_prepare_step (affine = 0) followed by cxk_take_step with the step length of
 * cone_program.cc:417-418, step = min(1, 2 / norminfd^2), evaluated ON THE DEVICE from the norms just
 * reduced -- so TakeStep is enqueued before the host waits for `info` and no idle gap separates the
 * two.  Same arithmetic, same bits as the two calls with the host computing the step.  *took = 1
 * when TakeStep was enqueued; 0 on configurations where a kernel needs the value from the host
 * (sharded contexts, equality constraints, LMI orders beyond LDS): the caller then runs
 * cxk_take_step itself.  Only for iterations whose factorization outcome is already known. */
int cxk_prepare_take_step(cxk_context* ctx, double c_weight, double e_weight, double* info, int* took);
/* TakeStep (cone_program.h:92-97) */
int cxk_take_step(cxk_context* ctx, int affine, double e_weight, double step_size);
/* GetWeightedSlackEigenvalues (cone_program.cc:31-57) on the device-resident y;
 * out = {lambda_min, lambda_max, frobenius_norm_squared, trace} */
int cxk_weighted_slack_eigenvalues(cxk_context* ctx, double c_weight, double* out);

/* ---- The barrier parameter selected on the device: one iteration of conex::Solve without the host
 * round trip between the eigenvalue query and the Newton direction (cone_program.cc:366-413).
 * The eigenvalue query's launch evaluates ComputeMuFromDivergence's rule and the update of
 * inv_sqrt_mu that Solve makes with it (cone_program.cc:166-224, :386-392, divergence.cc:17-110;
 * the same source as the host loop compiles: csrc/mu_rule.h -- the same IEEE operations, the same
 * bits) where the four reduced eigenvalue bounds appear; the Newton direction's right-hand side
 * (:409-411) and PrepareStep's c_weight (:413) then read inv_sqrt_mu from device memory, and the
 * host learns it -- with the factorization flag, the step norms and the by / cx scalars -- from the
 * ONE mailbox at the end of the iteration.  TakeStep, enqueued before the host has seen the
 * factorization's outcome, leaves W alone when the factorization failed.
 * cxk_device_mu_supported: 1 when this program can run that way -- one GPU, Cholesky on the device
 * (not the QR mode, no equality rows), no LMI beyond LDS (its TakeStep takes the step length from the
 * host) -- else 0.  Every cone type takes part: the selection rides in the tail workgroup of the
 * eigenvalue query where all constraints run on the register LMI kernels, in its reduction launch
 * otherwise. */
int cxk_device_mu_supported(cxk_context* ctx);
/* GetWeightedSlackEigenvalues(c_weight) on the device-resident y, then
 * inv_sqrt_mu <- limits(selection > 0 ? selection : prev / 2, lb, ub) on the device.  Does not wait. */
int cxk_select_mu_async(cxk_context* ctx, double c_weight, double divergence_upper_bound, int rank,
                        double prev, double lb, double ub);
/* cxk_newton_direction with k = the device's inv_sqrt_mu */
int cxk_newton_direction_device_mu(cxk_context* ctx, double b_scaling, double c_scaling);
/* The factorization carrying THREE right-hand sides through its one whole-tree launch -- bs b, cs AQc, AW --
 * so that the solve of the mu selection (K^-1 (-bs b + cs AQc), cone_program.cc:181: left in y) and the Newton
 * direction for the mu selected afterwards (K^-1 (k (bs b + cs AQc) - 2 AW), :409-411) are combinations of its
 * three solutions: the cxk_newton_direction_device_mu that follows is 3 N multiply-adds instead of a sweep
 * over the tree -- formed inside the PrepareStep launch that reads the direction, or by one elementwise launch
 * for whoever reads y before that (cxk_get_y, cxk_step_scalars, ...): the same values.  Call order:
 * cxk_assemble, cxk_factor_solve_triple_async, cxk_select_mu_async, cxk_newton_direction_device_mu,
 * cxk_prepare_take_step_device_mu.  cxk_triple_supported: 1 where that applies (the tree in one launch on one
 * GPU, every constraint on the register LMI kernels, the barrier parameter on the device, no refinement)
 * AND the assembly just enqueued still waits to ride in the factorization (ask directly behind cxk_assemble).
 * The three solutions hold for the b, W, slab and factor of that launch and for its b_scaling / c_scaling:
 * cxk_set_cost, cxk_set_W, cxk_set_identity, cxk_set_slab, cxk_assemble, cxk_factor(_async),
 * cxk_factor_solve_async, cxk_factor_direction_async and cxk_kkt_solve_async drop them (a direction already
 * asked for is formed first), and a cxk_newton_direction_device_mu with other scalings than the launch's solves
 * instead of combining them.  Solve-only sweeps (cxk_solve_rhs, cxk_newton_direction) and the queries keep them. */
int cxk_triple_supported(cxk_context* ctx);
int cxk_factor_solve_triple_async(cxk_context* ctx, double b_scaling, double c_scaling);
/* cxk_prepare_take_step with c_weight = the device's inv_sqrt_mu * c_scaling; waits, and returns
 * the selected inv_sqrt_mu as well */
int cxk_prepare_take_step_device_mu(cxk_context* ctx, double c_scaling, double e_weight, double* info,
                                    int* took, double* inv_sqrt_mu);

/* ---- inspection (tests, KKTMatrix() kkt_solver.cc:265-269) ------------- */
int cxk_get_slab(cxk_context* ctx, double* out);
int cxk_set_slab(cxk_context* ctx, const double* in);
/* G: the m x m Schur block of constraint i, column-major, G_ab = tr(A_a W A_b W) (symmetric for non-symmetric
 * A too).  On the device the block's contract is its lower triangle (row >= column): that is all the
 * factorization reads, and the matrix-inequality routes write nothing else.  The call returns that triangle
 * mirrored into the full symmetric square, never what lies above the diagonal on the device. */
int cxk_get_constraint_schur(cxk_context* ctx, int i, double* G /* m*m */, double* AW,
                             double* AQc, double* scalars /* 2 */);
int cxk_get_residuals(cxk_context* ctx, double* AW /* V */, double* AQc /* V: original variable order */,
                      double* scalars /* 2 */);

/* ---- multi-GPU (the reference is single process, so no counterpart) ----------
 * After cxk_set_shard(rank, world) + cxk_finalize every rank holds the same symbolic analysis
 * and the same deterministic partition: the elimination tree is cut at a level; everything
 * above the cut (the "top") is replicated, the subtrees below are dealt to ranks (longest
 * processing time first), each constraint lives with the subtree that eliminates it.
 * One KKT solve is then
 *     cxk_kkt_local_async   assemble own constraints, factor + forward-solve own subtrees,
 *                           fold their updates into the partial top, pack the exchange buffer
 *     all-reduce(sum) of the exchange buffer across ranks (RCCL; a few KB: latency bound)
 *     cxk_kkt_finish_async  unpack, factor/solve the top (replicated), back-substitute own
 *                           subtrees
 * after which a rank holds y for its own and for the top variables (cxk_get_valid_variables). */
/* Collectives.  With a communicator attached EVERY entry point of this header works on a sharded
 * context exactly as on a single-GPU one -- cxk_kkt_solve_async, cxk_factor*_async, cxk_solve_rhs,
 * cxk_newton_direction, cxk_solve_inplace (local sweep, ONE sum all-reduce of the top's share,
 * top, back-substitution), cxk_prepare_step / cxk_weighted_slack_eigenvalues / cxk_step_scalars /
 * cxk_line_search (scalar sum / max / min all-reduces), cxk_get_y (the whole vector) -- so the host
 * IPM loop (CONEX_Maximize) runs unchanged, every rank taking the same decisions from the same
 * reduced scalars.  The sums that cross ranks are those of supernodal_assembler.cc:103-111,162-164
 * (separator overlaps into the Schur system) and block_triangular_operations.cc:209-215 (Schur
 * updates of eliminated subtrees).
 *   cxk_comm_unique_id      ncclGetUniqueId on one rank; ship the 128 bytes to the others
 *   cxk_comm_init_rccl      ncclCommInitRank for this context's device (one process per GPU);
 *                           implies cxk_set_shard(rank, world) when called before cxk_finalize.
 *                           librccl.so is loaded on demand: single-GPU users need no RCCL
 *   cxk_comm_set_allreduce  any other transport / tests: in-place all-reduce of `count` doubles of
 *                           DEVICE memory, op 0 sum, 1 max, 2 min; work enqueued on `stream` before
 *                           the call must be seen and the result must be in place on return */
typedef int (*cxk_allreduce_fn)(void* user, double* device_buffer, long count, int op, void* stream);
int cxk_comm_unique_id(void* out128);
int cxk_comm_init_rccl(cxk_context* ctx, const void* unique_id128, int rank, int world_size);
int cxk_comm_set_allreduce(cxk_context* ctx, cxk_allreduce_fn fn, void* user);
/* diagnostic: a ONE-rank RCCL communicator on a context sharded as part of a larger (virtual) world:
 * the sharded step with real ncclAllReduce calls on a single GPU (results: one shard's only) */
int cxk_comm_init_rccl_solo(cxk_context* ctx);
/* sum / max / min all-reduces of `count` doubles through the RCCL communicator, checked */
int cxk_comm_selftest(cxk_context* ctx, int count);
/* ranks of the attached RCCL communicator as RCCL counts them (ncclCommCount); 0 without one */
int cxk_comm_count(const cxk_context* ctx);

/* SupernodalKKTSolver::SetSolverMode (kkt_solver.h:41; SolverConfiguration::kkt_solver): 0 / 1 the
 * supernodal LLT / LDLT (chosen by the structure, as kkt_solver.cc:180-193 does), 2
 * CONEX_QR_FACTORIZATION -- the reference's debugging mode for rank-deficient systems: Factor()
 * forms the dense N x N KKT matrix and takes its column-pivoted Householder QR, every solve goes
 * through it (kkt_solver.cc:175-178, 196-198, 227-231).  As there, this is dense host arithmetic on
 * one core (the assembled slab travels to the host at Factor, right-hand sides at every solve);
 * N is limited to 1500, single GPU. */
int cxk_set_solver_mode(cxk_context* ctx, int mode);

/* ---- per-phase device timers ------------------------------------------------------------
 * The reference brackets Assemble / Factor / Solve / Update of every iteration with START_TIMER /
 * END_TIMER (debug_macros.h:18-52; cone_program.cc:338-341, 359-372, 412-414, 421-437) when built
 * with CONEX_ENABLE_TIMER.  Here the caller marks the START of a phase; a hipEvent is recorded on
 * the context's stream (nothing waits), the device time up to the next mark is charged to that
 * phase, CXK_PHASE_OTHER collects what the reference leaves untimed (mu selection).
 * cxk_phase_read waits for the last mark, folds finished intervals and returns microseconds per
 * phase accumulated since the last reset.  CONEX_Maximize uses them when CONEX_ENABLE_TIMER=1 is
 * in the environment and prints the reference's "Assemble(us): .., Factor(us): .., ..." fields. */
enum { CXK_PHASE_ASSEMBLE = 0, CXK_PHASE_FACTOR = 1, CXK_PHASE_SOLVE = 2, CXK_PHASE_UPDATE = 3,
       CXK_PHASE_OTHER = 4, CXK_PHASE_COUNT = 5 };
int cxk_phase_timers(cxk_context* ctx, int on);
int cxk_phase_mark(cxk_context* ctx, int phase);
int cxk_phase_read(cxk_context* ctx, double* us /* CXK_PHASE_COUNT */, int reset);

/* The two halves of a sharded KKT solve, for callers that run the all-reduce themselves: */
int cxk_exchange_buffer(cxk_context* ctx, void** dev_ptr, long* count /* doubles */);
int cxk_exchange_download(cxk_context* ctx, double* out);   /* host copy, tests */
int cxk_exchange_upload(cxk_context* ctx, const double* in);
int cxk_kkt_local_async(cxk_context* ctx, double inv_sqrt_mu, double b_scaling, double c_scaling);
int cxk_kkt_finish_async(cxk_context* ctx, double inv_sqrt_mu, double b_scaling, double c_scaling);
int cxk_owns_constraint(const cxk_context* ctx, int i);
int cxk_get_valid_variables(const cxk_context* ctx, unsigned char* mask /* V, original variable order */);
int cxk_shard_info(const cxk_context* ctx, int* cut_level, int* num_levels, long* exchange_count);
/* single-GPU building blocks kept for symmetry with the reference call sequence */
int cxk_assemble_local(cxk_context* ctx);
int cxk_finish_assemble(cxk_context* ctx);

/* per-constraint {normsqrd, norminfd} of the last cxk_prepare_step (the StepInfo info_i of
 * cone_program.h:69-90 before the reduction); diagnostics and tests */
int cxk_get_step_info(cxk_context* ctx, double* out2k);

/* ComputeMuFromLineSearch (cone_program.cc:118-160) with PerformLineSearch / FindMinimumMu of the
 * linear cone (linear_constraint.cc:48-103): two solves with the current factorization (right-hand
 * sides -2 AW and AQc c_s + b b_s - 2 AW), per-row admissible interval of the step, reduced over
 * constraints.  *result = inv_sqrt_mu candidate, or -1 (a cone without line-search support --
 * constraint.h:24-28 -- or an empty interval).  Overwrites y. */
int cxk_line_search(cxk_context* ctx, double dinf_upper_bound, double b_scaling, double c_scaling,
                    double* result);

/* ---- isolated batched fp64 GEMM on the matrix pipe ----------------------------------------
 * C[b] = alpha op(A[b]) op(B[b]) + beta C[b], packed column-major host buffers (A is M x K, or
 * K x M when ta; B is K x N, or N x K when tb).  This is the kernel behind the large-order LMI
 * assembly (Eigen GEMM call sites dense_lmi_constraint.cc:72-103, psd_constraint.cc:13-28,45-84)
 * and the blocked supernode updates (block_triangular_operations.cc:184-219: LLT trailing update
 * and off^T off); exported so tests can check it and bench tools can time it against the fp64
 * MFMA roofline at the supernode sizes SURVEY 8(d) names.  lower_only: SYRK-shaped output
 * (m >= n).  splits > 1: split-K with an ordered reduction.  avg_ms: device time per launch. */
int cxk_gemm_f64(int device, int ta, int tb, int M, int N, int K, int batch, const double* A,
                 const double* B, double* C, double alpha, double beta, int lower_only, int splits,
                 int reps, double* avg_ms);

/* The same product on the operand layouts the library's own call sites pass (test entry).  `arena` (arena_len
 * doubles) is copied to ONE device allocation, the product runs once, and the whole arena is copied back.  f[32]
 * describes the call, offsets in doubles into the arena (so operands may alias, interleave, or sit 8 bytes off
 * alignment):
 *    0 M   1 N   2 K   3 ta   4 tb   5 batch   6 inner   7 lower_only   8 splits
 *    9 ordered: with splits > 1, 1 = partials then the ordered reduction into C, 0 = raw partials only (C unused)
 *   10 tile override (64 | 128 | 12864, the meaning of CXK_GEMM_TILE; 0 = the process's)   11 general-kernel override
 *   12 offset of A  13 lda  14 sA1  15 sA2     16 offset of B  17 ldb  18 sB1  19 sB2
 *   20 offset of C  21 ldc  22 sC1  23 sC2     24 offset of Ct (-1: none)  25 ldct  26 sT1  27 sT2  28 ctb  29 sTb
 *   30 offset of the split partials (-1: none)  31 sCs
 * Batch member z uses strides (z / inner, z % inner); Ct[n + m ldct + (n / ctb) sTb] = alpha (A B)(m, n).
 * A layout whose footprints (each operand and C for every batch member and split, from the first element to
 * (columns - 1) ld + rows behind it, an operand's rows counted up to the next even number; the image of C in
 * Ct) leave the arena, a negative stride, or a combination the launchers refuse (Ct with lower_only, Ct
 * with the ordered reduction) returns CXK_FAILURE before any launch.  *route: the kernel the call ran on. */
#define CXK_GEMM_ROUTE_GENERAL 0    /* gemm_f64_mfma */
#define CXK_GEMM_ROUTE_DMA16 1      /* gemm_f64_dma<16> */
#define CXK_GEMM_ROUTE_DMA32 2      /* gemm_f64_dma<32> */
#define CXK_GEMM_ROUTE_DMA128X128 3 /* gemm_f64_dma128<4> */
#define CXK_GEMM_ROUTE_DMA128X64 4  /* gemm_f64_dma128<2> */
int cxk_gemm_f64_layout(int device, double* arena, long long arena_len, const long long* f, double alpha,
                        double beta, int* route);

/* Number of (owned) LMI / Hermitian constraints evaluated from their nonzeros instead of dense
 * matrices (kernels_lmi_sparse.hip.h).  The C-ABI fills matrix inequalities
 * entry by entry (CONEX_UpdateLinearOperator, hermitian_psd.cc:249-275), so their A_i are
 * typically very sparse; cxk_initialize picks the sparse evaluation per constraint when its
 * (sum nnz)^2 / 2 terms cost less than the dense formula 4 n^3 (m+1) + n^2 m^2 (measured
 * break-even ratios in kernels_lmi_sparse.hip.h; CXK_SPARSE_LMI=0/1 in the environment forces
 * never/always).  Results equal the dense path's to rounding. */
int cxk_count_sparse_lmi(const cxk_context* ctx);

/* Number of (owned) LMI / Hermitian constraints whose Schur complement
 * (ConstructSchurComplementSystem, dense_lmi_constraint.cc:72-103) is evaluated by kernel `which`:
 * 0 literal LDS kernel (lmi_schur_generic; also every constraint with non-symmetric data, which
 * the reference accepts and evaluates as written), 1 row-per-lane DPP + MFMA kernel
 * (lmi_schur_fused), 2 persistent MFMA producer/consumer kernel (lmi_schur_mfma), 3 batched GEMM
 * pipeline (orders beyond LDS and mid-size orders), 4 sparse evaluation. */
int cxk_count_lmi_kernel(const cxk_context* ctx, int which);

/* The kernel instance each per-constraint stage of LMI / Hermitian constraint `constraint` runs, as
 * codes 0 .. cxk_lmi_kernel_count() - 1 in out[stage] (stages below).  The launches choose through
 * the same functions.  Fails for a constraint of another type, one not owned by this rank, or before
 * initialize.  One instance is no row of that list because it runs only where it was asked for: the Schur stage of
 * a sparse LMI whose affine term is evaluated from its nonzeros (cxk_set_sparse_affine) reports the code
 * cxk_lmi_kernel_count() + 1, which cxk_lmi_kernel_name names "lmi_schur_sparse hbm sparse-C".  Likewise
 * the folded forms of the five sparse instances (cxk_set_sparse_fold): codes cxk_lmi_kernel_count() + 2 .. + 6, named
 * as the instance with the suffix " folded". */
enum {
  CXK_LMI_STAGE_SCHUR = 0,   /* Schur complement assembly */
  CXK_LMI_STAGE_PREPARE = 1, /* PrepareStep */
  CXK_LMI_STAGE_QUERY = 2,   /* the weighted slack eigenvalue query */
  CXK_LMI_STAGE_TAKE = 3,    /* TakeStep */
  CXK_LMI_STAGE_AFFINE = 4   /* PrepareStep's affine update */
};
int cxk_lmi_kernels(const cxk_context* ctx, int constraint, int out[5]);
/* name of a code of cxk_lmi_kernels (null outside the range): kernel, template order, variant */
const char* cxk_lmi_kernel_name(int code);
int cxk_lmi_kernel_count(void);

/* Columns of the dense range at the top of the elimination tree (0 = none): when the last levels
 * hold a supernode of 33..64 columns and at most 64 columns in total, BlockCholeskyInPlace and
 * the block solves (block_triangular_operations.cc:114-219) restricted to those levels run as one
 * dense register factorization (kernels_kkt_top.hip.h) instead of supernode by supernode. */
int cxk_dense_top_columns(const cxk_context* ctx);

/* 1 when cxk_kkt_solve_async folds the assembly (UpdateBlocks / Scatter of
 * supernodal_assembler.cc:93-181 and the right-hand side of cone_program.cc:409-411) into the
 * launch of the first factor level: the leaves of the elimination tree read their panels straight
 * from the Schur blocks, the gather of everything else rides beside them as extra workgroups
 * (tree_factor_level_asm).  Decided per structure at cxk_finalize (Cholesky, the first
 * level one register shape, every supernode in it fed by exactly one constraint); results are the
 * bits of the separate assembly launch.  CXK_NO_FUSED_ASM=1 keeps the separate launch. */
int cxk_fused_assembly(const cxk_context* ctx);
/* 1 when a KKT solve (assembly gather + factorization + solve) runs as ONE launch over the whole
 * elimination tree (tree_fused.hip); CXK_NO_FUSED_TREE=1 in the environment turns it off */
int cxk_fused_tree(const cxk_context* ctx);
/* The pair of register frames (NSMAX << 8 | SMAX each, *frame_a <= *frame_b) the whole-tree launch runs its supernodes
 * in; zeros when cxk_fused_tree is 0.  cxk_finalize picks the tightest compiled pair that holds every supernode;
 * CXK_FUSED_PADDED_FRAMES=1 in the environment keeps the frames of the level kernels (speed only: same bits). */
int cxk_fused_tree_frames(const cxk_context* ctx, int* frame_a, int* frame_b);
/* The whole-tree launch keeps every supernode's wavefront resident and lets it wait, inside the
 * kernel, for its descendants' values: deadlock-free while the launch has the device to itself
 * (grid <= resident slots, workgroups dispatched in index order), every wait bounded.  On a device
 * shared with other streams or processes a wait can run out.  That is not a failed factorization:
 * the context then gives the whole-tree launch up for good and sweeps level by level (kernel
 * boundaries instead of in-kernel waits).  cxk_sync redoes the pending factor-and-solve that way
 * itself when that factor-and-solve was the last call before it; when anything else was called in
 * between (a solve-only sweep, the mu selection, a direction, PrepareStep, new inputs) it reports
 * failure instead, as cxk_factor_status always does.  After such a failure this function returns 1
 * ONCE, so that the caller (the interior-point loop of program.cc) redoes its sequence instead of
 * giving up. */
int cxk_fused_tree_timed_out(cxk_context* ctx);
/* Sharded contexts (cxk_set_shard, world > 1) must take the same branch on every rank, so a time-out
 * is settled the same way on all of them (the next entry point, cxk_factor_status or cxk_sync does it):
 *   - a wait of a rank's up launch (its own subtrees, before the exchange) ran out: it travels with the
 *     exchange buffer, so every rank reports a failed factorization, every rank's
 *     cxk_fused_tree_timed_out returns 1, and every rank sweeps level by level from then on (the same
 *     collectives as the whole-tree launches).  Nothing is redone silently.
 *   - a wait of a rank's top launch (behind the exchange) ran out and a solve sweep or a step reduction
 *     (eigenvalue query, PrepareStep) went out behind it: that collective carries a time-out mark in one
 *     extra slot, and every rank reports it as above.
 *   - a wait of a rank's top launch ran out and no collective went out behind it: that rank redoes its
 *     top and the way back down its subtrees on the level kernels, from the exchange buffer it holds and
 *     without a collective, and reports success; it sweeps level by level from then on.  cxk_get_y and
 *     cxk_line_search, whose gathers carry no mark, settle such a launch first.  The step-scalar
 *     all-reduce carries no mark either: when only it went out behind the launch the rank redoes the same
 *     way and warns that what it sent came from the timed-out launch (the interior-point loop always
 *     issues a step reduction before it asks for the factorization's outcome).
 * A sharded context makes no solve-only whole-tree sweep. */
/* test hook: pretend the latest whole-tree launch reported a wait that ran out */
int cxk_debug_force_fused_timeout(cxk_context* ctx);
/* test hook, one context at a time: the whole-tree factor launch number `launch_index` from now (0: the
 * next one) reports, behind its launch `which`, what a wait that ran out reports -- the failure word
 * d_fail[1] = the launch's tag on the device and the pinned host word -- and nothing else; no wait runs out.  which =
 * CXK_DEBUG_FUSED_FACTOR (single GPU: the factor-and-solve launch; what CXK_DEBUG_FUSED_TIMEOUT_AT=k set
 * at cxk_create does), CXK_DEBUG_FUSED_SHARD_UP or CXK_DEBUG_FUSED_SHARD_TOP (sharded: the launch before
 * or after the exchange).  The host word is raised before the launching call returns; with
 * CXK_DEBUG_FUSED_STREAM_ORDERED or'ed into CXK_DEBUG_FUSED_SHARD_TOP, by a host function on the stream
 * instead, as late as a launch still running when the host goes on raises it.  launch_index < 0 disarms
 * it.  Fails when the context makes no such launch. */
enum { CXK_DEBUG_FUSED_FACTOR = 0, CXK_DEBUG_FUSED_SHARD_UP = 1, CXK_DEBUG_FUSED_SHARD_TOP = 2,
       CXK_DEBUG_FUSED_STREAM_ORDERED = 16 };
int cxk_debug_fused_timeout_at(cxk_context* ctx, int launch_index, int which);

/* ---- timing / roofline accounting -------------------------------------- */
/* algorithmic bytes and flops of one dense-LMI assembly launch (SURVEY 8d formulas) */
int cxk_assembly_work(const cxk_context* ctx, double* bytes, double* flops);
/* average device time (ms) of the dominant assembly kernel since the last reset, measured
 * with hipEvents on the context's stream; returns number of samples */
int cxk_kernel_time(cxk_context* ctx, int reset, double* avg_ms);
/* the same for the other kernels of a Newton step (bench.py's `roofline_tree` and `newton_step`):
 * which = CXK_CLOCK_ASSEMBLY (what cxk_kernel_time reads), _TREE the tree launch(es) of a
 * factor-and-solve, _SOLVE a solve-only sweep, _QUERY the eigenvalue query, _PREPARE, _TAKE.  A slot
 * that is one kernel carries the event pair on its dispatch (the kernel's own begin / end time
 * stamps); a slot of several launches is bracketed and includes their boundaries
 * (DESIGN.md section 6 lists which slot is which at every configuration). */
enum { CXK_CLOCK_ASSEMBLY = 0, CXK_CLOCK_TREE = 1, CXK_CLOCK_SOLVE = 2, CXK_CLOCK_QUERY = 3,
       CXK_CLOCK_PREPARE = 4, CXK_CLOCK_TAKE = 5, CXK_CLOCK_COUNT = 6 };
int cxk_kernel_clock(cxk_context* ctx, int which, int reset, double* avg_ms);
/* on = 0: off; on = 1: bracket every launch of that kernel with a hipEvent pair; on = P > 1:
 * every P-th launch (an event pair costs a few us of stream time, sampling keeps the timed
 * region representative) */
/* SupernodalKKTSolver::SetIterativeRefinementIterations (kkt_solver.h:37, loop kkt_solver.cc:233-261):
 * the next factorization keeps the assembled matrix, and every solve after it runs `iterations`
 * steps y <- y + K^-1 (b - K y) on the device (supernodal mat-vec; the reference multiplies a
 * dense N x N copy).  0 switches it off.  Single GPU. */
int cxk_set_iterative_refinement(cxk_context* ctx, int iterations);

int cxk_enable_timing(cxk_context* ctx, int on);

#ifdef __cplusplus
}
#endif
#endif
