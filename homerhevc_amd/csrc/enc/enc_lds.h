// A worker's LDS: the one description.  A workgroup of the CTU kernels (k_encode.hip) is a row worker - wavefront 0 - and its helper wavefront, and its dynamic LDS
// is laid out here and nowhere else: every offset and every total is computed below, and the accessors behind them are how a kernel gets at a piece.
//
//   Work             the worker's windows, buffers and candidate lists (enc_types.h)
//   nodes            the worker's fast copy of the CTU's partition nodes (NODE_SLOTS of them)
//   helper scratch   the helper wavefront's own: 2 x 1024 coefficients - a 32 x 32 chroma TU - and a chroma neighbour array.  Behind Work and the nodes, so that
//                    the post-decision stage and task S, which run between two CTUs when the helper has no job, can use the three as one scratch area
//   Seq, FrameCtx    copies of the sequence and frame parameters, which are read all through the control code
//   mailbox          HelperBox (enc_common.h)
//   Enc x 2          the worker's context, then the helper's copy of it
//   WorkRd           the RD_FULL arrays: the tail, which a launch without RD_FULL pictures leaves out (a fourth worker then fits a CU)
//   timer table      profiling build only (-DHENC_PROFILE): ticks, then calls, per primitive class
//
// Two things that used to sit here do not any more, so that more workers fit a CU: the CTU's side-info record (the worker reads and writes it in HBM: measured in
// round 2 to make no difference) and the TU tables (FastTables: transform bases, scans, quantiser cells - from DevTables through L2 instead: 1-2 % per worker,
// against twice the workers).  The partition geometry, whose place the helper's scratch has, is in constant memory (enc_common.h GeoTable).
#pragma once
#include "enc_types.h"

// Primitive-level timers of the profiling build (-DHENC_PROFILE, device only): lane 0 adds s_memtime ticks and a call count per primitive class
// to the timer table of the worker's LDS (PRIM_END, enc_prims.h); the kernels fold it into the per-row profile.
enum { PP_SAD = 0, PP_SSD, PP_BLK, PP_FILLREF, PP_ADIFILT, PP_INTRAPRED, PP_INTERP, PP_TRF, PP_TRI, PP_QUANT, PP_DEQUANT, PP_CAND, PP_SYNC, PP_INFO, PP_CTU_IO, PP_HWAIT, PP_COUNT };

namespace henc {

// Of the CTU's 341 partition nodes a worker keeps the 21 of depths 0 .. 2 and the depth-3 and depth-4 nodes (16 + 64) of ONE quadrant (the 32 x 32 area of a
// depth-1 node) in its fast memory: the walks are depth first, so while a depth-1 node and what hangs below it is evaluated no deeper node of another quadrant is
// touched (the checker build verifies exactly that at every access; the one exception, the corner units of the 64 x 64 CU, is handled where it occurs); the other
// three quadrants' nodes wait in the CTU's record in HBM (nodes_select_quad).
constexpr int NODES_RESIDENT = 21, NODES_D3 = 85, NODE_QUAD_D3 = 16, NODE_QUAD_D4 = 64, NODE_SLOTS = NODES_RESIDENT + NODE_QUAD_D3 + NODE_QUAD_D4;
constexpr int HSCRATCH_ELEMS = 2048 + 144;                     // int16 of the helper's scratch
constexpr int LDS_BOX_BYTES = 160, LDS_ENC_BYTES = 272;      // what the mailbox and a context may take (checked behind HelperBox / Enc, enc_common.h)
constexpr int LDS_WAVES = 2;                                   // wavefronts of a workgroup: the worker and its helper, a context each

constexpr int lds_up16(size_t bytes) { return (int)((bytes + 15) & ~(size_t)15); }
constexpr int LDS_OFF_WORK = 0;
constexpr int LDS_OFF_NODES = LDS_OFF_WORK + lds_up16(sizeof(Work));
constexpr int LDS_OFF_HSCRATCH = LDS_OFF_NODES + lds_up16(sizeof(Node) * NODE_SLOTS);
constexpr int LDS_OFF_SEQ = LDS_OFF_HSCRATCH + HSCRATCH_ELEMS * 2;
constexpr int LDS_OFF_FRAME = LDS_OFF_SEQ + lds_up16(sizeof(Seq));
constexpr int LDS_OFF_BOX = LDS_OFF_FRAME + lds_up16(sizeof(FrameCtx));
constexpr int LDS_OFF_ENC = LDS_OFF_BOX + LDS_BOX_BYTES;
constexpr int LDS_OFF_RD = LDS_OFF_ENC + LDS_WAVES * LDS_ENC_BYTES;
constexpr int LDS_OFF_PROF = (LDS_OFF_RD + lds_up16(sizeof(WorkRd)) + 1023) & ~1023;      // (the next multiple of 1 KiB behind everything else)
// the three totals: with the RD_FULL arrays, without them, and the profiling build's
constexpr int LDS_FULL_BYTES = LDS_OFF_RD + lds_up16(sizeof(WorkRd)), LDS_LEAN_BYTES = LDS_OFF_RD, LDS_PROF_BYTES = LDS_OFF_PROF + 2 * PP_COUNT * 8;
// what a launch asks for (needs_rd: one of its pictures at least is RD_FULL)
constexpr int lds_request(bool needs_rd)
{
#if defined(HENC_PROFILE)
	(void)needs_rd;
	return LDS_PROF_BYTES;
#else
	return needs_rd ? LDS_FULL_BYTES : LDS_LEAN_BYTES;
#endif
}
static_assert(LDS_OFF_NODES % 16 == 0 && LDS_OFF_HSCRATCH % 16 == 0 && LDS_OFF_SEQ % 16 == 0 && LDS_OFF_FRAME % 16 == 0 && LDS_OFF_BOX % 16 == 0 && LDS_OFF_ENC % 16 == 0 && LDS_OFF_RD % 16 == 0,
	      "every piece of a worker's LDS starts at a multiple of 16 bytes");
static_assert(LDS_OFF_RD == LDS_LEAN_BYTES && LDS_FULL_BYTES <= LDS_OFF_PROF, "the RD_FULL arrays are the tail of a worker's LDS: launches without RD_FULL pictures leave them out; the timer table lies behind them");
static_assert(LDS_PROF_BYTES <= 160 * 1024, "a workgroup has 160 KiB of LDS on gfx950");

#if defined(__HIPCC__)
// The pieces of the LDS of the workgroup that asks.  Each accessor but the helpers' is a constant: it takes no argument, so that the compiler knows the address before
// it decides anything else - a worker's context that every caller of the walk takes from lds_enc() is a constant inside the walk's functions too (with one accessor
// for all contexts and the wavefront as its argument it was not, and the P-slice walk came out 1.3 % larger).
// (The kernels and their set-up code reach the dynamic LDS under this name, the LDS members of Enc - LdsAt, enc_platform.h - under a second one, as they always have.)
extern __shared__ __align__(16) unsigned char henc_lds[];
struct Enc;
struct HelperBox;
__device__ __forceinline__ Work *lds_work() { return (Work *)(henc_lds + LDS_OFF_WORK); }
__device__ __forceinline__ Node *lds_nodes() { return (Node *)(henc_lds + LDS_OFF_NODES); }
__device__ __forceinline__ int16_t *lds_helper_scratch() { return (int16_t *)(henc_lds + LDS_OFF_HSCRATCH); }
__device__ __forceinline__ Seq *lds_seq() { return (Seq *)(henc_lds + LDS_OFF_SEQ); }
__device__ __forceinline__ FrameCtx *lds_frame() { return (FrameCtx *)(henc_lds + LDS_OFF_FRAME); }
__device__ __forceinline__ HelperBox *lds_box() { return (HelperBox *)(henc_lds + LDS_OFF_BOX); }
__device__ __forceinline__ Enc &lds_enc() { return *(Enc *)(henc_lds + LDS_OFF_ENC); }                                 // the worker's context
__device__ __forceinline__ Enc &lds_helper_enc(int h) { return *(Enc *)(henc_lds + LDS_OFF_ENC + (1 + h) * LDS_ENC_BYTES); }      // helper h's copy
__device__ __forceinline__ unsigned long long *lds_prof() { return (unsigned long long *)(henc_lds + LDS_OFF_PROF); }
// everything below `bytes` starts from zero, on the `threads` lanes that call (LDS keeps what the last workgroup on the CU left in it)
__device__ __forceinline__ void lds_zero(unsigned bytes, int tid, int threads)
{
	for (int i = tid; i < (int)(bytes / 4); i += threads) ((uint32_t *)henc_lds)[i] = 0;
}
#endif

}  // namespace henc
