// What the units of the per-cone stages call in one another.  kkt_cone_launch.hip drives every stage as an exhaustive
// switch over Group::route; each arm is one call into the unit that owns the route's kernels:
//   cone_linear.hip  kLinearLds, kLinearTiled, kLinearSparse; vec_set_identity, the Gram product and the nonzero lists
//                    that other vector cones use too
//   cone_soc.hip     kSocLds, kSocStreamed, kSocSparse; soc_stream_slack, which the streamed quadratic cones run too
//   cone_quad.hip    kQuadLds, kQuadStreamed
//   cone_lmi.hip     kLmiDense, kLmiSparse, kLmiFactored; the list of LMI kernel instances and its choosers
// (kOct and kStatic are one launch per stage and stay in kkt_cone_launch.hip.)  Each unit holds the views of its routes
// (Make*), their stages of cxk_finalize (Upload*) and their launches, and is the only one to touch its family's member
// of Group (lin, soc, quad, lmi: cone_state.h, which lists the exceptions); `mode` of a PrepareStep / query call is 0 or 1 and
// picks the <0> / <1> instance of the kernels.  Host declarations only, no device code.  Everything is hidden
// (CXK_LOCAL) but the functions libconex.so has always exported: those keep their visibility.
#pragma once
#include <hip/hip_ext.h>

#include "cone_types.h"
#include "kkt_launch.h"

namespace cxk {
struct QuadStreamGroup;  // kernels_quad_stream.hip.h
struct QuadStreamVecs;
}  // namespace cxk

namespace cxk_host {

// ---- kkt_cone_launch.hip
// Kernel clocks (CXK_CLOCK_*): a slot whose launches are ONE register kernel carries the event pair on that
// dispatch; anything else is bracketed by event records around its launches.
struct StepClock {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool sample = false, on_dispatch = false;
};
CXK_LOCAL StepClock BeginStepClock(cxk_context* ctx, int slot, bool one_register_kernel);
CXK_LOCAL void EndStepClock(cxk_context* ctx, const StepClock& c);
// The assembly clock around the launches of one group, for the scope it is declared in.
struct CXK_LOCAL AssemblyClock {
  cxk_context* ctx;
  StepClock clk;
  explicit AssemblyClock(cxk_context* c, bool on_dispatch = false) : ctx(c), clk(BeginStepClock(c, CXK_CLOCK_ASSEMBLY, on_dispatch)) {}
  ~AssemblyClock() { EndStepClock(ctx, clk); }
};
#define CXK_LAUNCH_CLOCKED(clk, kernel, grid, block, ...)                                                        \
  do {                                                                                                           \
    if ((clk).on_dispatch)                                                                                       \
      hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, ctx->stream, (clk).e0, (clk).e1, 0, __VA_ARGS__); \
    else                                                                                                         \
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, ctx->stream, __VA_ARGS__);                          \
  } while (0)

// ---- cone_linear.hip
VecGroup MakeVec(Group& g);
CXK_LOCAL void LinearNonzeros(ConstraintRec* c);
CXK_LOCAL int AllocLinearT2(cxk_context* ctx, Group& g);  // UploadGroup: every group, ahead of its route's stage
// the group's nonzeros into `nz` (its family's lists): second-order cones on the sparse route too
CXK_LOCAL int UploadSparseNonzeros(cxk_context* ctx, const Group& g, NonzeroLists& nz);
// Gf = alpha WA' WA of every member, and its work space: streamed second-order cones too
CXK_LOCAL int AllocGramWorkspace(cxk_context* ctx, GramWs& w, size_t cnt, size_t len, size_t m, const FinalizeSwitches& sw);
CXK_LOCAL hipError_t LaunchGramLower(const GramWs& w, const double* WA, double* Gf, int cnt, int len, int m, double alpha, hipStream_t st);
CXK_LOCAL int UploadLinearTiled(cxk_context* ctx, Group& g, const FinalizeSwitches& sw);
CXK_LOCAL int UploadLinearSparse(cxk_context* ctx, Group& g);
CXK_LOCAL void LaunchLinearLdsSchur(Group& g, const Arena& ar, hipStream_t st);
hipError_t LaunchLinearTiledSchur(Group& g, const Arena& ar, hipStream_t st);
hipError_t LaunchLinearSparseSchur(Group& g, const Arena& ar, hipStream_t st);
CXK_LOCAL int LaunchLinearPrepare(cxk_context* ctx, Group& g, int mode, const StepArgs& sa);
CXK_LOCAL void LaunchLinearTakeStep(Group& g, const StepArgs& sa, hipStream_t st);
CXK_LOCAL int LaunchLinearGroupLineSearch(cxk_context* ctx, Group& g, const LineSearchArgs& a);
CXK_LOCAL void LaunchVecSetIdentity(Group& g, bool soc, hipStream_t st);  // second-order and quadratic cones: soc

// ---- cone_soc.hip
CXK_LOCAL hipError_t RaiseSocLdsLimits();
CXK_LOCAL int UploadSocStream(cxk_context* ctx, Group& g, const FinalizeSwitches& sw);
CXK_LOCAL int UploadSocSparse(cxk_context* ctx, Group& g);
CXK_LOCAL void LaunchSocLdsSchur(cxk_context* ctx, Group& g, const Arena& ar);
hipError_t LaunchSocStreamSchur(Group& g, const Arena& ar, hipStream_t st);
hipError_t LaunchSocSparseSchur(Group& g, const Arena& ar, hipStream_t st);
CXK_LOCAL int LaunchSocPrepare(cxk_context* ctx, Group& g, int mode, const StepArgs& sa);
CXK_LOCAL int LaunchSocTakeStep(cxk_context* ctx, Group& g, const StepArgs& sa);
// soc_stream_slack on the rows of d.v into d.ms (the streamed quadratic cones: QuadStreamSlackView)
CXK_LOCAL void LaunchSocStreamSlack(const SocStreamGroup& d, const StepArgs& sa, hipStream_t st);
// soc_sparse_slack on the rows of `nz` (those of v) into ms (the quadratic cones held by the nonzeros of A)
CXK_LOCAL void LaunchSocSparseSlack(const VecGroup& v, double* ms, const NonzeroLists& nz, const StepArgs& sa, hipStream_t st);

// ---- cone_quad.hip
CXK_LOCAL hipError_t RaiseQuadLdsLimits();
CXK_LOCAL int UploadQuadGram(cxk_context* ctx, Group& g);
CXK_LOCAL int UploadQuadStream(cxk_context* ctx, Group& g, const FinalizeSwitches& sw);
// a kQuadStreamed group whose Q is held by its parts (Group::quad.sq.on): instead of UploadQuadStream
CXK_LOCAL int UploadQuadStructured(cxk_context* ctx, Group& g, const FinalizeSwitches& sw);
// ... and its pass out_r = Q x_r, which LaunchQuadStreamQmv hands over (defined behind it, in the same unit)
template <int R>
CXK_LOCAL hipError_t LaunchQuadStructuredQmv(Group& g, const cxk::QuadStreamGroup& d, const cxk::QuadStreamVecs& x, hipStream_t st);
// a kQuadStreamed group whose A is held by its nonzeros (Group::quad.sa.on): the nonzeros and row 0, ahead of either
// Upload above, which then form the constants from them (QuadSparseConstants)
CXK_LOCAL int UploadQuadSparseA(cxk_context* ctx, Group& g);
CXK_LOCAL int QuadSparseConstants(cxk_context* ctx, Group& g);
// v (and, with a dense A, u) of an assembly: quad_stream_schur_columns, or quad_sparse_columns through the CSC
CXK_LOCAL void LaunchQuadSchurColumns(Group& g, const cxk::QuadStreamGroup& d, hipStream_t st);
CXK_LOCAL void LaunchQuadLdsSchur(Group& g, const Arena& ar, hipStream_t st);
hipError_t LaunchQuadStreamSchur(Group& g, const Arena& ar, hipStream_t st);
CXK_LOCAL int LaunchQuadPrepare(cxk_context* ctx, Group& g, int mode, const StepArgs& sa);
CXK_LOCAL int LaunchQuadTakeStep(cxk_context* ctx, Group& g, const StepArgs& sa);

// ---- cone_lmi.hip
CXK_LOCAL hipError_t RaiseLmiLdsLimits();
// GroupConstraints: what Choose asks about a dense-added LMI (mfma_supports, sparse_pays)
CXK_LOCAL void MeasureLmi(const ConstraintRec& c, ConeShape* s);
// a constraint on kLmiSparse evaluates its affine term from C's nonzeros under `mode` (-1 / 0 / 1: cxk_set_sparse_affine)
CXK_LOCAL bool LmiTakesSparseAffine(const ConstraintRec& c, int mode, double min_ratio);
// UploadGroup: the group's assembly, whether it is `large`, and the work space of the chip-wide Lanczos run
CXK_LOCAL int PlanLmiGroup(cxk_context* ctx, Group& g, const FinalizeSwitches& sw);
CXK_LOCAL int UploadLmiDense(cxk_context* ctx, Group& g, const FinalizeSwitches& sw);
CXK_LOCAL int UploadLmiSparse(cxk_context* ctx, Group& g);
CXK_LOCAL int UploadLmiFactored(cxk_context* ctx, Group& g);
CXK_LOCAL LmiAssembly LmiAssemblyOf(const Group& g);   // cxk_count_lmi_kernel
CXK_LOCAL bool LmiOnWideSpectrum(const Group& g);      // cxk_count_wide_spectrum: its Lanczos runs take the chip-wide kernels
CXK_LOCAL bool LmiRowsServePrepare(const Group& g);  // lmi_prepare_rows has an instance for the group's shape
// the group's PrepareStep / query (pmode: LmiPrepareKernel's) or TakeStep is one launch of a rows kernel
CXK_LOCAL bool LmiPrepareOnRows(const cxk_context* ctx, const Group& g, int pmode);
CXK_LOCAL bool LmiTakeOnRows(const Group& g);
CXK_LOCAL int LaunchLmiDenseSchur(cxk_context* ctx, Group& g, const Arena& ar);
CXK_LOCAL int LaunchLmiSparseSchur(cxk_context* ctx, Group& g, const Arena& ar);
CXK_LOCAL int LaunchLmiFactoredSchur(cxk_context* ctx, Group& g, const Arena& ar);
// tail_blocks: what the tail workgroup adds to the grid of lmi_prepare_rows; clk: on its dispatch when clk.on_dispatch
CXK_LOCAL int LaunchLmiPrepare(cxk_context* ctx, Group& g, int mode, int pmode, const StepArgs& sa, const StepTail& tail,
                               int tail_blocks, const StepClock& clk);
CXK_LOCAL int LaunchLmiTakeStep(cxk_context* ctx, Group& g, const StepArgs& sa, const StepClock& clk);
CXK_LOCAL void LaunchLmiSetIdentity(Group& g, hipStream_t st);

}  // namespace cxk_host
