/*
 * homer_gpu.h - C ABI of the MI355X (gfx950) backend for HomerHEVC's per-block encode hot path.
 *
 * The reference's plug-in surface is `struct low_level_funcs_t` (hmr_private.h:1063-1092), a table of
 * 19 function pointers filled once in HOMER_enc_init (hmr_encoder_lib.c:155-214).  This library
 * replaces what is behind that table, plus the in-loop kernels the reference keeps outside it
 * (deblock, SAO offset, intra reference build, border padding), with hand-written HIP
 * kernels.  Three layers, all `extern "C"`, plain pointers and sizes:
 *
 *   1. context / device memory          hmr_gpu_create ... hmr_gpu_timer_stop
 *   2. drop-in entries                   hmr_gpu_sad(...) etc.: HOST pointers, synchronous, the exact
 *                                        low_level_funcs_t signatures (henc_thread_t* arguments flattened
 *                                        to the scalars they carry); one launch per call - correct, not fast
 *   3. batched entries                   hmr_gpu_*_batch(ctx, jobs, n, ...): DEVICE-resident planes addressed by
 *                                        job descriptors; one launch per batch - the performance path
 *      frame-level in-loop passes        hmr_gpu_deblock_frame / sao_* / pad_frame
 *   test aids (sections 15 - 17)         the walk's primitives one call at a time (15), its device-only forms on a synthetic worker (16),
 *                                        the post-decision stage of one picture from given CTU records (17: hmr_gpu_enc_post_records)
 *
 * All samples are int16_t and strides are in elements, as in the reference.
 * Every entry returns 0 on success or a negative hmr_gpu_status; nothing falls back to the CPU.
 */
#ifndef HOMER_GPU_H
#define HOMER_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hmr_gpu_ctx hmr_gpu_ctx;

enum hmr_gpu_status {
	HMR_GPU_OK = 0,
	HMR_GPU_ERR_NO_DEVICE = -1,   /* no HIP device / wrong architecture */
	HMR_GPU_ERR_HIP = -2,         /* a HIP call failed, see hmr_gpu_last_error */
	HMR_GPU_ERR_ARG = -3,         /* unsupported size or malformed argument */
	HMR_GPU_ERR_NOMEM = -4
};

/* ------------------------------------------------------------------------------------------------
 * 1. context, device memory, timing
 * ------------------------------------------------------------------------------------------------ */

/* Create a context on `device` (HIP ordinal).  `stream` may be an existing hipStream_t (e.g. the
 * torch current stream, passed as void*) or NULL to let the context own one. */
int hmr_gpu_create(hmr_gpu_ctx **out, int device, void *stream);
void hmr_gpu_destroy(hmr_gpu_ctx *ctx);
const char *hmr_gpu_last_error(void);
int hmr_gpu_sync(hmr_gpu_ctx *ctx);
void *hmr_gpu_stream(hmr_gpu_ctx *ctx);   /* the hipStream_t every launch of this context goes to */

int hmr_gpu_malloc(hmr_gpu_ctx *ctx, void **dev_ptr, size_t bytes);
int hmr_gpu_free(hmr_gpu_ctx *ctx, void *dev_ptr);
int hmr_gpu_upload(hmr_gpu_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);     /* sync */
int hmr_gpu_download(hmr_gpu_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);   /* sync */
int hmr_gpu_memset(hmr_gpu_ctx *ctx, void *dev_dst, int value, size_t bytes);

/* An empty launch on the context's stream (timing calibration: what an event pair around a launch costs besides the kernel). */
int hmr_gpu_nop(hmr_gpu_ctx *ctx);
/* VALU issue probe: blocks * 4 wavefronts, each issuing iters * 8 independent packed dot products and nothing else (out: any device word, never written in
 * practice).  bench.py times it to state the integer issue rate the kernels are priced against as measured on the box, next to the nominal one. */
int hmr_gpu_valu_probe(hmr_gpu_ctx *ctx, int kind, int blocks, int iters, uint32_t *out);   /* kind 0: v_dot2_i32_i16, 1: v_sad_u16 */
/* Cap on the workgroups of one batched launch (process-wide, default 4096).  Batched kernels grid-stride over their jobs, so results do not
 * depend on it; lower it to leave compute units to concurrent streams. */
int hmr_gpu_set_max_grid(int blocks);

/* HIP-event timer on the context's stream (bench.py brackets the timed region with it). */
int hmr_gpu_timer_start(hmr_gpu_ctx *ctx);
int hmr_gpu_timer_stop(hmr_gpu_ctx *ctx, float *elapsed_ms);   /* records, synchronises, returns ms */
/* explicit event pairs on the same stream, for per-kernel durations (elapsed() is valid once ev1 has completed) */
int hmr_gpu_event_create(hmr_gpu_ctx *ctx, void **ev);
int hmr_gpu_event_record(hmr_gpu_ctx *ctx, void *ev);
int hmr_gpu_event_elapsed(void *ev0, void *ev1, float *elapsed_ms);
int hmr_gpu_event_destroy(void *ev);

/* Constant tables the kernels use, built at context creation (defaults of hmr_tables.c:62,221 and
 * hmr_encoder_lib.c:93-140); exposed so the host can check them against its own. */
int hmr_gpu_get_scan_table(int scan_mode, int log2_size, uint32_t *out);          /* (1<<log2)^2 entries */
int hmr_gpu_get_quant_table(int log2_size, int list, int rem, int32_t *quant, int32_t *dequant);

/* ------------------------------------------------------------------------------------------------
 * 2. drop-in entries: host pointers, synchronous.  Signatures = low_level_funcs_t members
 *    (hmr_private.h:1066-1091); they run on the process-wide default context (device 0, created on
 *    first use, or the one set with hmr_gpu_set_default).
 * ------------------------------------------------------------------------------------------------ */
int hmr_gpu_set_default(hmr_gpu_ctx *ctx);

/* hmr_private.h:1066-1068 (sse_copy_16_16 / sse_copy_16_8 / sse_copy_8_16), SSE impl hmr_sse42_functions_pixel.c:152,319,236 */
void hmr_gpu_copy_16_16(void *src, uint32_t src_stride, void *dst, uint32_t dst_stride, int height, int width);
void hmr_gpu_copy_16_8(void *src, uint32_t src_stride, void *dst, uint32_t dst_stride, int height, int width);
void hmr_gpu_copy_8_16(void *src, uint32_t src_stride, void *dst, uint32_t dst_stride, int height, int width);
/* :1069 sad, :1071 ssd16b, :1072 predict, :1073 reconst, :1074 modified_variance */
uint32_t hmr_gpu_sad(int16_t *src, uint32_t src_stride, int16_t *pred, uint32_t pred_stride, int size);
uint32_t hmr_gpu_ssd16b(int16_t *src, uint32_t src_stride, int16_t *pred, uint32_t pred_stride, int size);
void hmr_gpu_predict(int16_t *orig, int orig_stride, int16_t *pred, int pred_stride, int16_t *residual, int residual_stride, int size);
void hmr_gpu_reconst(int16_t *pred, int pred_stride, int16_t *residual, int residual_stride, int16_t *decoded, int decoded_stride, int size);
uint32_t hmr_gpu_modified_variance(int16_t *p, int size, int stride, int modif);
/* :1076 create_intra_planar_prediction, :1077 create_intra_angular_prediction (henc_thread_t*, ctu_info_t* dropped:
 * they only carry scratch buffers, the angle tables and ctu->top/left which are always 1, hmr_motion_intra.c:257) */
void hmr_gpu_intra_planar(int16_t *prediction, int pred_stride, int16_t *adi_pred_buff, int adi_size, int cu_size);
void hmr_gpu_intra_angular(int16_t *prediction, int pred_stride, int16_t *adi_pred_buff, int adi_size, int cu_size, int cu_mode, int is_luma);
/* not in the table: fill_reference_samples hmr_motion_intra.c:246 and adi_filter :189, partition node flattened to flags */
void hmr_gpu_fill_reference_samples(int16_t *decoded_corner, int stride, int n, int left, int top, int bottom_left, int top_right,
				    int bl_size, int tr_size, int16_t *adi_out);
void hmr_gpu_adi_filter(int16_t *adi, int16_t *out, int adi_size, int n, int strong_enabled);
/* :1079-1081 interpolate_luma_m_compensation/_m_estimation, interpolate_chroma_m_compensation, :1083 weighted_average_motion */
void hmr_gpu_interpolate_luma(int16_t *reference_buff, int reference_buff_stride, int16_t *pred_buff, int pred_buff_stride, int fraction,
			      int width, int height, int is_vertical, int is_first, int is_last);
void hmr_gpu_interpolate_chroma(int16_t *reference_buff, int reference_buff_stride, int16_t *pred_buff, int pred_buff_stride, int fraction,
				int width, int height, int is_vertical, int is_first, int is_last);
void hmr_gpu_weighted_average(int16_t *src0, int src0_stride, int16_t *src1, int src1_stride, int16_t *dst, int dst_stride, int height, int width);
/* :1088 transform, :1089 itransform (bit depth fixed at 8, uiMode reduced to "DST-VII for 4x4 intra luma") */
void hmr_gpu_transform(int16_t *block, int16_t *coeff, int block_stride, int n, int is_dst);
void hmr_gpu_itransform(int16_t *block, int16_t *coeff, int block_stride, int n, int is_dst);
/* :1085 quant, :1086 inv_quant.  henc_thread_t* replaced by what it is read for: slice type (hmr_sse42_functions_quant.c:47),
 * pps->sign_data_hiding_flag (:121) and the aux_buff scratch that receives deltaU (:48; NULL = do not return it). */
void hmr_gpu_quant(int16_t *src, int16_t *dst, int16_t *delta_u, int scan_mode, int depth, int comp, int is_intra, int slice_is_intra,
		   int sign_hiding, int *ac_sum, int cu_size, int per, int rem);
void hmr_gpu_inv_quant(int16_t *src, int16_t *dst, int depth, int comp, int is_intra, int cu_size, int per, int rem);
/* :1091 get_sao_stats.  The henc_thread_t, slice_t and ctu_info_t pointers are replaced by what they are read for: the picture planes (HOST pointers to
 * sample (0,0), strides in elements), the picture size and the CTU's luma position; stats[comp][type][diff|count][32] as int64 like
 * sao_stat_data_t (hmr_private.h:455).  Only the CTU and its one-sample ring are transferred. */
void hmr_gpu_get_sao_stats(const int16_t *const orig[3], const int orig_stride[3], const int16_t *const recon[3], const int recon_stride[3], int pict_width,
			   int pict_height, int ctu_x, int ctu_y, int64_t *stats);

/* In-loop filters at the reference's own call granularity, HOST pointers (planes address sample (0,0), strides in elements; unit arrays are raster over
 * the picture's 4x4 units like hmr_gpu_units; unit_flags = HMR_GPU_UNIT_INTRA | HMR_GPU_UNIT_CBF_Y).  Only the CTU's neighbourhood is transferred.
 * hmr_deblock_filter_cu (hmr_deblocking_filter.c:737), sao_offset_ctu (hmr_sao.c:1210), reference_picture_border_padding_ctu (hmr_encoder_lib.c:1723). */
void hmr_gpu_deblock_filter_ctu(int16_t *const planes[3], const int strides[3], int width, int height, int units_stride, const int16_t *mvx, const int16_t *mvy,
				const int8_t *ref_idx, const uint8_t *qp, const uint8_t *unit_flags, const uint8_t *pred_depth, const uint8_t *tr_idx, int ctu_x,
				int ctu_y, int ctu_size, int dir, int cb_qp_offset, int cr_qp_offset, int beta_offset_div2, int tc_offset_div2);
void hmr_gpu_sao_offset_ctu(const int16_t *const src[3], const int src_stride[3], int16_t *const dst[3], const int dst_stride[3], int width, int height, int ctu_x,
			    int ctu_y, const int32_t *params /* [3][34] = {modeIdc, typeIdc, offset[32]} per component */);
void hmr_gpu_pad_ctu(int16_t *const planes[3], const int strides[3], int width, int height, int pad_x, int pad_y, int ctu_x, int ctu_y, int ctu_size);

/* ------------------------------------------------------------------------------------------------
 * 3. batched entries: device-resident operands, one launch per call, asynchronous on the context's
 *    stream.  A job addresses up to three operands by ELEMENT offset from the base pointer passed to
 *    the call; all jobs of one call share `size` (the host groups work by block size, the way it
 *    groups CUs by depth).  `jobs` is a DEVICE pointer (upload with hmr_gpu_upload).
 * ------------------------------------------------------------------------------------------------ */
typedef struct hmr_gpu_job {
	uint32_t a_off, a_stride;   /* first operand  (src / orig / pred / reference / adi / coeff-in)  */
	uint32_t b_off, b_stride;   /* second operand (pred / residual / ...)                            */
	uint32_t c_off, c_stride;   /* output                                                            */
	uint16_t w, h;              /* extent where the kernel is not square (copies, interpolation)    */
	uint32_t p0, p1;            /* kernel-specific parameters, see each entry                        */
} hmr_gpu_job;

/* out[i] = SAD / SSD of job i.  a = src, b = pred (b_stride may be 0 for ssd) */
int hmr_gpu_sad_batch(hmr_gpu_ctx *ctx, const hmr_gpu_job *jobs, int njobs, int size, const int16_t *a_base, const int16_t *b_base, uint32_t *out);
int hmr_gpu_ssd16b_batch(hmr_gpu_ctx *ctx, const hmr_gpu_job *jobs, int njobs, int size, const int16_t *a_base, const int16_t *b_base, uint32_t *out);
/* c = a - b */
int hmr_gpu_predict_batch(hmr_gpu_ctx *ctx, const hmr_gpu_job *jobs, int njobs, int size, const int16_t *a_base, const int16_t *b_base, int16_t *c_base);
/* c = clip(a (pred) + b (residual, stride may be 0)) */
int hmr_gpu_reconst_batch(hmr_gpu_ctx *ctx, const hmr_gpu_job *jobs, int njobs, int size, const int16_t *a_base, const int16_t *b_base, int16_t *c_base);
/* c[h x w] = a[h x w]; kind 0: i16->i16, 1: u8->i16, 2: i16->u8 (offsets/strides in elements of each side's type).
 * kind | N << 8 promises that every job is an N x N int16 square (N = 4, 8, 16, 32, 64): vectorised fast path. */
int hmr_gpu_copy_batch(hmr_gpu_ctx *ctx, const hmr_gpu_job *jobs, int njobs, int kind, const void *a_base, void *c_base);
/* out[i] = modified variance of the size x size block at a; p0 = modif */
int hmr_gpu_modified_variance_batch(hmr_gpu_ctx *ctx, const hmr_gpu_job *jobs, int njobs, int size, const int16_t *a_base, uint32_t *out);
/* a = adi array (4*size+1 entries at a_off), c = prediction; p0 = cu_mode (0 planar, 1 DC, 2..34), p1 = is_luma */
int hmr_gpu_intra_pred_batch(hmr_gpu_ctx *ctx, const hmr_gpu_job *jobs, int njobs, int size, const int16_t *a_base, int16_t *c_base);
/* a = reconstructed plane, a_off addresses the corner sample (-1,-1), c = adi out (4*size+1), b_off = filtered adi out;
 * p0 bits: 0 left, 1 top, 2 bottom_left, 3 top_right, 4 write filtered copy, 5 strong filter enabled; p1 = bl_size | tr_size << 16 */
int hmr_gpu_intra_refs_batch(hmr_gpu_ctx *ctx, const hmr_gpu_job *jobs, int njobs, int size, const int16_t *a_base, int16_t *c_base);
/* a = reference/intermediate, c = out, w/h = extent; p0 = fraction, p1 bits: 0 vertical, 1 first, 2 last.
 * flags bit 0: luma (8 taps) / chroma (4 taps); bits 8..15: lanes-per-job hint 4 / 8 / 16 / 32 / 64 (0 = 64).  A job is
 * ceil(w/4)*ceil(h/4) work items when vertical (4x4 outputs from a register window of rows) or ceil(w/8)*h when
 * horizontal (8 outputs per item); that many lanes share it, so batches of small blocks should pass a small hint. */
int hmr_gpu_interpolate_batch(hmr_gpu_ctx *ctx, const hmr_gpu_job *jobs, int njobs, int flags, const int16_t *a_base, int16_t *c_base);
int hmr_gpu_weighted_average_batch(hmr_gpu_ctx *ctx, const hmr_gpu_job *jobs, int njobs, const int16_t *a_base, const int16_t *b_base, int16_t *c_base);
/* a = residual block (strided), c = coefficients (linear size*size at c_off); p0 = is_dst */
int hmr_gpu_transform_batch(hmr_gpu_ctx *ctx, const hmr_gpu_job *jobs, int njobs, int size, const int16_t *a_base, int16_t *c_base);
/* a = coefficients (linear), c = residual block (strided); p0 = is_dst */
int hmr_gpu_itransform_batch(hmr_gpu_ctx *ctx, const hmr_gpu_job *jobs, int njobs, int size, const int16_t *a_base, int16_t *c_base);
/* a = coefficients in, c = levels out (both linear), b_off = deltaU out when delta_u_base != NULL;
 * p0 bits 0-1 scan_mode, 2-3 comp, 4 is_intra, 5 slice_is_intra, 6 sign_hiding; p1 = per | rem << 8; ac_sum[i] out */
int hmr_gpu_quant_batch(hmr_gpu_ctx *ctx, const hmr_gpu_job *jobs, int njobs, int size, const int16_t *a_base, int16_t *c_base,
			int16_t *delta_u_base, int32_t *ac_sum);
/* a = levels, c = coefficients; p0 bits 2-3 comp, 4 is_intra; p1 = per | rem << 8 */
int hmr_gpu_inv_quant_batch(hmr_gpu_ctx *ctx, const hmr_gpu_job *jobs, int njobs, int size, const int16_t *a_base, int16_t *c_base);


/* ------------------------------------------------------------------------------------------------
 * 4. frame-level in-loop passes (the reference keeps these outside the table and runs them CTU by CTU in a
 *    lagged pipeline, hmr_encoder_lib.c:2386 hmr_deblock_sao_pad_sync_ctu; whole-picture passes are
 *    equivalent).  All pointers are DEVICE pointers; launches are asynchronous on the context's stream.
 * ------------------------------------------------------------------------------------------------ */
typedef struct hmr_gpu_frame {
	int width, height;          /* luma size, multiples of 8 (hmr_encoder_lib.c:1001) */
	int16_t *y, *u, *v;         /* sample (0,0) of each plane; margins, if any, lie before/after */
	int stride_y, stride_c;     /* elements */
} hmr_gpu_frame;

/* side-info the encoder decided, one entry per 4x4 luma unit in raster order (ctu_info_t arrays of
 * hmr_private.h:792-843 are the same data in z-order per CTU) */
#define HMR_GPU_UNIT_INTRA 1     /* pred_mode == INTRA_MODE */
#define HMR_GPU_UNIT_CBF_Y 2     /* CBF(ctu, idx, Y_COMP, tr_idx) */
#define HMR_GPU_UNIT_EDGE_VER 4  /* left edge of the unit is a transform/CU edge (set by hmr_gpu_edge_flags_frame) */
#define HMR_GPU_UNIT_EDGE_HOR 8  /* top edge */
typedef struct hmr_gpu_units {
	int units_stride;           /* units per row of the arrays below */
	const int16_t *mvx, *mvy;   /* mv_ref[REF_PIC_LIST_0], quarter-sample units */
	const int8_t *ref_idx;      /* mv_ref_idx[REF_PIC_LIST_0], < 0 = none */
	const uint8_t *qp;
	uint8_t *flags;
} hmr_gpu_units;

/* The same side-info as the encoder keeps it: per CTU, 256 entries in z-order (ctu_info_t: mv_ref[0], mv_ref_idx[0], qp, pred_mode, cbf[Y_COMP],
 * pred_depth, tr_idx), CTU-major.  hmr_gpu_units_from_ctus re-orders it on the device into the raster arrays above (abs2raster_table,
 * hmr_encoder_lib.c:95-100; flags = INTRA | CBF_Y at the unit's tr_idx) plus raster pred_depth / tr_idx for hmr_gpu_edge_flags_frame. */
typedef struct hmr_gpu_ctu_units {
	const int16_t *mvx, *mvy;
	const int8_t *ref_idx;
	const uint8_t *qp, *pred_mode, *cbf_y, *pred_depth, *tr_idx;
} hmr_gpu_ctu_units;
int hmr_gpu_units_from_ctus(hmr_gpu_ctx *ctx, const hmr_gpu_ctu_units *src, int ctus_x, int ctus_y, const hmr_gpu_units *dst, uint8_t *pred_depth_raster,
			    uint8_t *tr_idx_raster);

/* derive the EDGE bits of flags[] from the coding tree: pred_depth + tr_idx per unit (hmr_deblocking_filter.c:737-825) */
int hmr_gpu_edge_flags_frame(hmr_gpu_ctx *ctx, const uint8_t *pred_depth, const uint8_t *tr_idx, int width, int height, int units_stride, uint8_t *flags);
/* hmr_deblock_filter_cu over the picture (hmr_deblocking_filter.c:737): boundary strength, luma strong/weak, chroma; in place.
 * bs_ver / bs_hor (optional, units_stride x height/4) receive 0x80|bs for every evaluated edge segment. P/I slices. */
int hmr_gpu_deblock_frame(hmr_gpu_ctx *ctx, const hmr_gpu_frame *frame, const hmr_gpu_units *info, int cb_qp_offset, int cr_qp_offset,
			  int beta_offset_div2, int tc_offset_div2, uint8_t *bs_ver, uint8_t *bs_hor);
/* hmr_deblock_filter_cu's own granularity (hmr_deblocking_filter.c:737): the edges of one direction (0 = EDGE_VER, 1 = EDGE_HOR, hmr_private.h:122)
 * inside the CTU at luma position (ctu_x, ctu_y).  pred_depth / tr_idx (optional, DEVICE, raster like the unit arrays): when given, the EDGE bits of
 * the CTU's units are derived first. */
int hmr_gpu_deblock_ctu(hmr_gpu_ctx *ctx, const hmr_gpu_frame *frame, const hmr_gpu_units *info, const uint8_t *pred_depth, const uint8_t *tr_idx,
			int cb_qp_offset, int cr_qp_offset, int beta_offset_div2, int tc_offset_div2, int ctu_x, int ctu_y, int ctu_size, int dir);
/* low_level_funcs_t.get_sao_stats (hmr_private.h:1091, hmr_sse42_sao.c:35) for every CTU:
 * stats[ctu][comp][type EO0,EO90,EO135,EO45,BO][0 = diff, 1 = count][32] as int32 */
int hmr_gpu_sao_stats_frame(hmr_gpu_ctx *ctx, const hmr_gpu_frame *orig, const hmr_gpu_frame *recon, int32_t *stats);
/* the same for one CTU (the table's call granularity); stats[comp][type][diff|count][32] */
int hmr_gpu_sao_stats_ctu(hmr_gpu_ctx *ctx, const hmr_gpu_frame *orig, const hmr_gpu_frame *recon, int ctu_index, int32_t *stats);
/* sao_offset_ctu (hmr_sao.c:1210) for every CTU: src = pre-SAO picture, dst = output (must hold a copy of src);
 * params[ctu][comp][34] = {modeIdc, typeIdc, offset[32]} */
int hmr_gpu_sao_apply_frame(hmr_gpu_ctx *ctx, const hmr_gpu_frame *src, const hmr_gpu_frame *dst, const int32_t *params);
/* the same for one CTU (sao_offset_ctu's own granularity); params = that CTU's [3][34] */
int hmr_gpu_sao_apply_ctu(hmr_gpu_ctx *ctx, const hmr_gpu_frame *src, const hmr_gpu_frame *dst, int ctu_index, const int32_t *params);
/* reference_picture_border_padding_ctu (hmr_encoder_lib.c:1723) for every CTU: replicate edges into pad_x/pad_y (luma; chroma half) */
int hmr_gpu_pad_frame(hmr_gpu_ctx *ctx, const hmr_gpu_frame *frame, int pad_x, int pad_y);


/* ------------------------------------------------------------------------------------------------
 * 5. motion: search driver and compensation (the reference's L3 helpers that sit directly on the kernels)
 * ------------------------------------------------------------------------------------------------ */
/* One PU of hmr_motion_estimation (hmr_motion_inter.c:1404).  Vectors are in quarter samples. */
typedef struct hmr_gpu_me_job {
	double corr;                 /* calc_mv_correction(qp, avg_dist) = qp * clip(avg_dist / 2000., .15, 1.4), hmr_common.h:53 (host-side double) */
	uint32_t orig_off, orig_stride;   /* source block */
	uint32_t ref_off, ref_stride;     /* co-located block (mv = 0) in the padded reference picture */
	int16_t gx, gy;              /* curr_part_global_x / _y */
	int16_t init_x, init_y;      /* start vector, integer samples */
	int16_t n_amvp, n_search;    /* candidate counts: AMVP list (vector cost, 1..2), search list et->mv_search_candidates (0..5) */
	int16_t amvp[2][2];
	int16_t search[5][2];
	uint32_t action;             /* MOTION_PEL_MASK 1 | MOTION_HALF_PEL_MASK 2 | MOTION_QUARTER_PEL_MASK 4, hmr_common.h:77-79 */
	uint32_t reserved;
} hmr_gpu_me_job;
typedef struct hmr_gpu_me_result {
	int32_t mvx, mvy;            /* *mv */
	int32_t subx, suby;          /* *subpix_mv */
	uint32_t sad;                /* return value */
} hmr_gpu_me_result;
/* jobs / out are DEVICE arrays; all PUs of a call share `size` (8, 16, 32, 64); range = MOTION_SEARCH_RANGE_X/Y (128/64, hmr_private.h:76-77).
 * The 16 sub-pel planes of hmr_half/quarter_pixel_estimation_luma_hm (hmr_motion_inter.c:395,442) are produced and consumed on chip. */
int hmr_gpu_motion_estimation_batch(hmr_gpu_ctx *ctx, const hmr_gpu_me_job *jobs, int njobs, int size, const int16_t *orig_base, const int16_t *ref_base,
				    int range_x, int range_y, int frame_w, int frame_h, hmr_gpu_me_result *out);
/* hmr_motion_compensation_luma / _chroma (hmr_motion_inter.c:1779,1860): a = co-located block, c = prediction, w/h extent,
 * p0 = mv.x, p1 = mv.y (as int32; quarter samples for luma, eighth samples for chroma).
 * flags bit 0: luma / chroma; bits 8..15: lanes-per-job hint 4 / 8 / 16 / 32 / 64 (0 = 64): that many lanes share a block of w*h samples (a work item is
 * four adjacent outputs; a two-stage block whose (h + taps - 1) x w first stage does not fit lanes/64 of the wave's LDS tile falls back to a slower form) */
int hmr_gpu_mc_batch(hmr_gpu_ctx *ctx, const hmr_gpu_job *jobs, int njobs, int flags, int is_bi_predict, const int16_t *a_base, int16_t *c_base);
/* host-pointer (drop-in) forms */
uint32_t hmr_gpu_motion_estimation(int16_t *orig, int orig_stride, int16_t *ref, int ref_stride, int gx, int gy, int init_x, int init_y, int size,
				   int range_x, int range_y, int frame_w, int frame_h, const int32_t *amvp, int n_amvp, const int32_t *search, int n_search,
				   double corr, int action, int32_t *out_mv4);
void hmr_gpu_mc_luma(int16_t *ref, int ref_stride, int16_t *pred, int pred_stride, int width, int height, int mvx, int mvy, int is_bi);
void hmr_gpu_mc_chroma(int16_t *ref, int ref_stride, int16_t *pred, int pred_stride, int size, int mvx, int mvy, int is_bi);


/* ------------------------------------------------------------------------------------------------
 * 6. command lists: one frame's launches described once, replayed from C (optionally as a hipGraph)
 * ------------------------------------------------------------------------------------------------ */
enum hmr_gpu_op {
	HMR_GPU_OP_SAD = 1, HMR_GPU_OP_SSD16B, HMR_GPU_OP_PREDICT, HMR_GPU_OP_RECONST, HMR_GPU_OP_COPY, HMR_GPU_OP_VARIANCE, HMR_GPU_OP_INTRA_PRED,
	HMR_GPU_OP_INTRA_REFS, HMR_GPU_OP_INTERPOLATE, HMR_GPU_OP_WAVG, HMR_GPU_OP_TRANSFORM, HMR_GPU_OP_ITRANSFORM, HMR_GPU_OP_QUANT,
	HMR_GPU_OP_INV_QUANT, HMR_GPU_OP_MC, HMR_GPU_OP_ME, HMR_GPU_OP_EDGE_FLAGS, HMR_GPU_OP_DEBLOCK, HMR_GPU_OP_SAO_STATS, HMR_GPU_OP_SAO_APPLY, HMR_GPU_OP_PAD,
	HMR_GPU_OP_TU_CHAIN,  /* jobs = hmr_gpu_tu_job*, a = orig base, b = pred base, c = level base, out = ssd; the reconstruction base and ac_sum follow in p64[0..1] */
	HMR_GPU_OP_INTRA_SEARCH,  /* jobs = hmr_gpu_intra_job*, a = orig base, b = decoded base, c = output base, out = hmr_gpu_intra_result* */
	HMR_GPU_OP_INTER_TU_CHAIN = 25, /* jobs = hmr_gpu_inter_tu_job*, a = residual base, b = pred base, c = level base, out = ssd; p64 = {recon base, ac_sum} */
	HMR_GPU_OP_SAO_OFFSETS = 30,    /* a = stats, njobs = CTUs, b = lambdas, c = offsets, out = aux, p64[0] = dist */
	HMR_GPU_OP_CHROMA_SEARCH = 29,  /* jobs = hmr_gpu_chroma_job*, a = orig base, b = decoded base, p64[0] = luma search results or NULL, out = hmr_gpu_intra_result* */
	HMR_GPU_OP_TU_MULTI = 28,       /* jobs = hmr_gpu_tu_segment* (host), njobs = segments, a = orig base, b = decoded base, c = level base, p64[0] = recon / prediction base */
	HMR_GPU_OP_PIXEL_MULTI = 27,    /* jobs = hmr_gpu_segment* (host), njobs = segments, size = HMR_GPU_OP_SAD / SSD16B / PREDICT / RECONST / COPY */
	HMR_GPU_OP_TREE_DECIDE = 26,    /* jobs = hmr_gpu_tree_job*, a = ssd, b = ac_sum, c = recon base, out = hmr_gpu_tree_result*; p64[0] = level base */
	HMR_GPU_OP_INTRA_TU_CHAIN = 24 /* jobs = hmr_gpu_itu_job*, a = orig base, b = decoded base, c = level base, out = ssd; p64 = {recon base, ac_sum, hmr_gpu_intra_result* or NULL};
	                           * the prediction plane shares the recon base; p[0] = rounds (0 / 1 = one set of jobs) */
};
/* One call of the batched / frame-level API: `size` is that entry's size/kind/flags argument, a/b/c/out its pointer arguments in
 * declaration order (frame-level ops take host pointers to hmr_gpu_frame / hmr_gpu_units that must outlive the list), p[] its
 * scalar arguments (deblock: cb, cr, beta, tc offsets; pad: pad_x, pad_y; edge flags: width, height, units_stride; ME: range_x,
 * range_y, frame_w, frame_h; MC: size = flags, p[0] = is_bi_predict).  QUANT: b = deltaU base (may be NULL), out = ac_sum. */
typedef struct hmr_gpu_cmd {
	int op, njobs, size;
	int p[4];
	const void *jobs, *a, *b;
	void *c, *out;
	void *p64[3];               /* extra pointer arguments (TU_CHAIN: recon base, ac_sum; INTRA_TU_CHAIN: + the search results when jobs take their mode from them) */
	int branch;                 /* 0 = the context's stream.  Commands with the same branch run in list order; different branches are
	                             * declared independent of each other and may overlap when the list is replayed as a graph (fork at the
	                             * start of the list, join at its end).  hmr_gpu_cmdlist_run ignores it (one stream, list order). */
} hmr_gpu_cmd;
#define HMR_GPU_MAX_BRANCHES 64
/* A context and its command lists belong to one host thread at a time (capture temporarily redirects the context's stream to the branch
 * streams); use one context per thread / per encoder engine. */
/* Several batches of ONE pixel kernel that differ only in the block size, in one launch: a frame's SAD (or SSD, residual, reconstruction, square int16
 * copy) batches are short launches that cannot fill the GPU one at a time.  op = HMR_GPU_OP_SAD / SSD16B / PREDICT / RECONST / COPY; every segment is what
 * the corresponding hmr_gpu_*_batch call takes (jobs = device array, size = block size, out = that batch's result array for SAD / SSD, ignored otherwise);
 * a, b, c as in the single-batch entries (COPY: a -> c).  Command lists: op HMR_GPU_OP_PIXEL_MULTI, size = the pixel op, jobs = host array of segments
 * (must outlive the list), njobs = number of segments. */
#define HMR_GPU_MAX_SEGMENTS 8
typedef struct hmr_gpu_segment {
	const hmr_gpu_job *jobs;
	void *out;
	int njobs, size;
} hmr_gpu_segment;
int hmr_gpu_pixel_multi(hmr_gpu_ctx *ctx, int op, const hmr_gpu_segment *segs, int nseg, const int16_t *a, const int16_t *b, int16_t *c);
/* The same for the fused TU chains of section 7: any mix of TU size (4, 8, 16, 32) and kind - 0 given prediction (hmr_gpu_tu_job), 1 intra (hmr_gpu_itu_job),
 * 2 inter (hmr_gpu_inter_tu_job) - as segments of one launch; all segments address the same five bases.  rounds / modes as in
 * hmr_gpu_intra_tu_chain_rounds_batch (0 / NULL when unused).  A launch that contains a 32x32 segment reserves that body's LDS image (52 KB per workgroup)
 * for every segment.  Command lists: op HMR_GPU_OP_TU_MULTI, jobs = host array of segments, njobs = number of segments, a = orig, b = decoded, c = level base,
 * p64[0] = recon / prediction base. */
struct hmr_gpu_intra_result;
typedef struct hmr_gpu_tu_segment {
	const void *jobs;
	uint32_t *ssd;
	int32_t *ac_sum;
	const struct hmr_gpu_intra_result *modes;
	int njobs, size, kind, rounds;
} hmr_gpu_tu_segment;
int hmr_gpu_tu_chain_multi(hmr_gpu_ctx *ctx, const hmr_gpu_tu_segment *segs, int nseg, const int16_t *orig_base, const int16_t *decoded_base, int16_t *pred_base,
			   int16_t *level_base, int16_t *recon_base);
typedef struct hmr_gpu_cmdlist hmr_gpu_cmdlist;
int hmr_gpu_cmdlist_create(hmr_gpu_ctx *ctx, const hmr_gpu_cmd *cmds, int n, hmr_gpu_cmdlist **out);
/* eager replay; event_pairs (optional, 2*n events from hmr_gpu_event_create) brackets every command for per-kernel timing */
int hmr_gpu_cmdlist_run(hmr_gpu_ctx *ctx, hmr_gpu_cmdlist *list, void **event_pairs);
/* capture the list into a hipGraph once, then launch the graph (a frame is a fixed launch sequence) */
int hmr_gpu_cmdlist_capture(hmr_gpu_ctx *ctx, hmr_gpu_cmdlist *list);
int hmr_gpu_cmdlist_replay(hmr_gpu_ctx *ctx, hmr_gpu_cmdlist *list);
void hmr_gpu_cmdlist_destroy(hmr_gpu_cmdlist *list);


/* ------------------------------------------------------------------------------------------------
 * 7. fused transform-unit chain: predict -> transform -> quant(+SBH) -> [inv_quant -> itransform] -> reconst -> ssd16b
 *    for a batch of TUs in one launch (the sequence of encode_intra_cu hmr_motion_intra.c:1014-1069 and
 *    encode_inter_cu hmr_motion_inter.c:40-230); bit-identical to the seven calls issued one after the other.
 * ------------------------------------------------------------------------------------------------ */
typedef struct hmr_gpu_tu_job {
	uint32_t orig_off, orig_stride;   /* source block */
	uint32_t pred_off, pred_stride;   /* prediction block */
	uint32_t rec_off, rec_stride;     /* reconstruction out */
	uint32_t lev_off;                 /* quantised levels out, linear size*size */
	uint32_t p0;                      /* bits 0-1 scan_mode, 2-3 comp, 4 is_intra, 5 slice_is_intra, 6 sign_hiding, 7 is_dst (4x4 intra luma) */
	uint32_t p1;                      /* per | rem << 8 */
} hmr_gpu_tu_job;
int hmr_gpu_tu_chain_batch(hmr_gpu_ctx *ctx, const hmr_gpu_tu_job *jobs, int njobs, int size, const int16_t *orig_base, const int16_t *pred_base,
			   int16_t *level_base, int16_t *recon_base, uint32_t *ssd, int32_t *ac_sum);
/* host-pointer (drop-in) form; returns the SSD between source and reconstruction */
uint32_t hmr_gpu_tu_chain(int16_t *orig, int orig_stride, int16_t *pred, int pred_stride, int16_t *levels, int16_t *recon, int recon_stride, int size,
			  int is_dst, int scan_mode, int comp, int is_intra, int slice_is_intra, int sign_hiding, int per, int rem, int *ac_sum);

/* The same chain for an intra TU, prediction included: encode_intra_cu's data path (hmr_motion_intra.c:1011-1068) - neighbour array from the plane
 * under reconstruction (smoothed when the host's is_filtered rule :1011-1012 says so), planar / DC / angular prediction, then the chain above.
 * The reconstruction may go back into the plane the neighbours are read from (the reference works in place); jobs of one call must not depend
 * on each other's reconstruction. */
typedef struct hmr_gpu_itu_job {
	uint32_t orig_off, orig_stride;   /* source block */
	uint32_t pred_off, pred_stride;   /* prediction out (prediction_wnd) */
	uint32_t rec_off, rec_stride;     /* reconstruction out */
	uint32_t lev_off;                 /* quantised levels out, linear size*size */
	uint32_t p0, p1;                  /* as hmr_gpu_tu_job (is_intra is implied) */
	uint32_t dec_off, dec_stride;     /* corner sample (-1,-1) of the block in the plane under reconstruction */
	uint32_t flags;                   /* bits 0 left, 1 top, 2 bottom_left, 3 top_right, 5 strong_intra_smooth_enabled, 6 is_filtered, 7 is_luma */
	uint32_t sizes;                   /* bl_size | tr_size << 16 */
	uint32_t mode;                    /* 0 planar, 1 DC, 2..34 angular */
} hmr_gpu_itu_job;
int hmr_gpu_intra_tu_chain_batch(hmr_gpu_ctx *ctx, const hmr_gpu_itu_job *jobs, int njobs, int size, const int16_t *orig_base, const int16_t *decoded_base,
				 int16_t *pred_base, int16_t *level_base, int16_t *recon_base, uint32_t *ssd, int32_t *ac_sum);
/* host-pointer (drop-in) form; returns the SSD between source and reconstruction.  `recon` may point into the plane `decoded_corner` belongs to. */
uint32_t hmr_gpu_intra_tu_chain(int16_t *orig, int orig_stride, int16_t *decoded_corner, int decoded_stride, int left, int top, int bottom_left, int top_right,
				int bl_size, int tr_size, int strong_enabled, int is_filtered, int mode, int is_luma, int16_t *pred, int pred_stride, int16_t *levels,
				int16_t *recon, int recon_stride, int size, int is_dst, int scan_mode, int comp, int slice_is_intra, int sign_hiding, int per, int rem,
				int *ac_sum);
/* As above with the prediction mode handed over ON THE DEVICE: a job whose flags carry bit 8 takes its mode from modes[job.mode].best_mode (the result
 * array of an intra search launched before it) and derives the smoothing rule (hmr_motion_intra.c:1011-1012) and the scan (find_scan_mode,
 * hmr_tables.c:398-402) from mode and TU size itself; is_filtered / scan_mode / mode of such a job are ignored.  A job with is_luma = 0 (chroma TU: its mode
 * comes from a chroma search, section 10) is never smoothed and takes the chroma scan rule (mode dependent for 4x4 only, hmr_tables.c:403-411); only the
 * low 8 bits of best_mode are the prediction mode. */
#define HMR_GPU_ITU_MODE_FROM_SEARCH 0x100u
struct hmr_gpu_intra_result;   /* section 8 */
int hmr_gpu_intra_tu_chain_modes_batch(hmr_gpu_ctx *ctx, const hmr_gpu_itu_job *jobs, int njobs, int size, const int16_t *orig_base, const int16_t *decoded_base,
				       int16_t *pred_base, int16_t *level_base, int16_t *recon_base, uint32_t *ssd, int32_t *ac_sum,
				       const struct hmr_gpu_intra_result *modes);
/* `rounds` sets of njobs jobs in one launch (jobs[r * njobs + j], ssd / ac_sum indexed the same way): job j of set r + 1 may read what job j of set r
 * reconstructed - the four children of a CU in z-order (hmr_motion_intra.c:1441-1477) run back to back on the same lanes instead of as four launches.
 * modes may be NULL when no job carries HMR_GPU_ITU_MODE_FROM_SEARCH. */
int hmr_gpu_intra_tu_chain_rounds_batch(hmr_gpu_ctx *ctx, const hmr_gpu_itu_job *jobs, int njobs, int rounds, int size, const int16_t *orig_base,
					const int16_t *decoded_base, int16_t *pred_base, int16_t *level_base, int16_t *recon_base, uint32_t *ssd, int32_t *ac_sum,
					const struct hmr_gpu_intra_result *modes);
/* The inter TU: encode_inter_cu / encode_inter_cu_chroma (hmr_motion_inter.c:40-230).  The residual of the motion-compensated CU is given; per TU: DCT,
 * quantisation as non-intra, and for a coded TU the keep-or-drop decision ssd_zero <= ssd + zero_thr * sum on SSDs in the residual domain, scaled by
 * `weight` and truncated to uint32 like the reference (luma: weight 1.0).  zero_thr = clip(avg_dist / 2.5 - 5, 1, 20000) (:59-60,108; host double).
 * Outputs: levels (zeros when dropped), reconstruction, ac_sum (0 when dropped), ssd = the residual-domain SSD of the coded candidate. */
typedef struct hmr_gpu_inter_tu_job {
	uint32_t orig_off, orig_stride;   /* RESIDUAL block (residual_wnd) */
	uint32_t pred_off, pred_stride;   /* prediction block */
	uint32_t rec_off, rec_stride;     /* reconstruction out */
	uint32_t lev_off;                 /* quantised levels out, linear size*size */
	uint32_t p0, p1;                  /* as hmr_gpu_tu_job (is_intra = 0, is_dst = 0) */
	uint32_t reserved;                /* bit 0 (HMR_GPU_INTER_TU_FROM_SOURCE): orig_off addresses the SOURCE block and the residual = source - prediction (16-bit wrap, the
	                                   * `predict` call the reference issues per CU ahead of encode_inter, hmr_motion_inter.c:3054-3056) is formed in the kernel */
	double weight, zero_thr;
} hmr_gpu_inter_tu_job;
#define HMR_GPU_INTER_TU_FROM_SOURCE 1u
int hmr_gpu_inter_tu_chain_batch(hmr_gpu_ctx *ctx, const hmr_gpu_inter_tu_job *jobs, int njobs, int size, const int16_t *residual_base, const int16_t *pred_base,
				 int16_t *level_base, int16_t *recon_base, uint32_t *ssd, int32_t *ac_sum);
uint32_t hmr_gpu_inter_tu_chain(int16_t *residual, int residual_stride, int16_t *pred, int pred_stride, int16_t *levels, int16_t *recon, int recon_stride, int size,
				int scan_mode, int comp, int slice_is_intra, int sign_hiding, int per, int rem, double weight, double zero_thr, int *ac_sum);

/* All inter TUs of one CU's transform tree (encode_inter, hmr_motion_inter.c:3069-3290: encode_inter_cu + encode_inter_cu_chroma per node, luma and both chroma
 * planes, parent and child level) in one submission, host pointers: inter TUs read only the CU's residual and prediction, so the tree can be computed ahead of
 * the walk that compares (cost < parent cost, :3211) and consolidates it.  In: the pointer / parameter fields; out: levels, recon, ssd, ac_sum of every entry. */
typedef struct hmr_gpu_inter_tu_host {
	int16_t *residual; int residual_stride;
	int16_t *pred; int pred_stride;
	int16_t *levels;
	int16_t *recon; int recon_stride;
	int size, scan_mode, comp, slice_is_intra, sign_hiding, per, rem;
	double weight, zero_thr;
	uint32_t ssd;
	int ac_sum;
} hmr_gpu_inter_tu_host;
void hmr_gpu_inter_tu_chain_n(hmr_gpu_inter_tu_host *tus, int n);

/* ------------------------------------------------------------------------------------------------
 * 8. intra mode search of one PU: homer_loop1_motion_intra (hmr_motion_intra.c:1084-1179) - reference build, smoothing,
 *    up to 13 {prediction, SAD} rounds over the search_points schedule (:1076) and the strict-< cost comparison
 *    SAD + bits * sqrt_lambda (double) in one launch.  The most-probable-mode list (get_intra_dir_luma_predictor,
 *    hmr_arithmetic_encoding.c:545) and the bit counts are host inputs: RD_FAST 1 / 12 (:1153-1157), RD_FULL the CABAC
 *    estimate of each list entry / 6 (:1141-1150), RD_DIST_ONLY 0 / 0.
 * ------------------------------------------------------------------------------------------------ */
typedef struct hmr_gpu_intra_job {
	double sqrt_lambda;               /* et->rd.sqrt_lambda */
	uint32_t orig_off, orig_stride;   /* source block */
	uint32_t dec_off, dec_stride;     /* corner sample (-1,-1) of the block in the plane under reconstruction */
	uint32_t adi_off, adif_off;       /* out: raw and smoothed neighbour arrays, 4*size+1 each (et->adi_pred_buff / adi_filtered_pred_buff) */
	uint32_t pred_off, pred_stride;   /* out: prediction of the LAST candidate evaluated (what the reference leaves in prediction_wnd) */
	uint32_t flags;                   /* bits 0 left, 1 top, 2 bottom_left, 3 top_right, 5 strong_intra_smooth_enabled */
	uint32_t sizes;                   /* bl_size | tr_size << 16 (hmr_motion_intra.c:289,335) */
	int32_t preds[3];                 /* most probable modes, -1 = none */
	uint32_t pred_bits[3];            /* bit count when the candidate equals preds[i] */
	uint32_t other_bits;              /* bit count of any other candidate */
	uint32_t reserved;
} hmr_gpu_intra_job;
typedef struct hmr_gpu_intra_result {
	int32_t best_mode;                /* best_pred_modes[0] */
	int32_t bits;                     /* return value: bit count of the best mode */
	double cost;                      /* best_pred_cost[0] */
} hmr_gpu_intra_result;
/* jobs / out are DEVICE arrays; all PUs of a call share `size` (4, 8, 16, 32, 64) */
int hmr_gpu_intra_search_batch(hmr_gpu_ctx *ctx, const hmr_gpu_intra_job *jobs, int njobs, int size, const int16_t *orig_base,
			       const int16_t *decoded_base, int16_t *out_base, hmr_gpu_intra_result *out);
/* host-pointer (drop-in) form; out = {best mode, bit count} */
void hmr_gpu_intra_search(int16_t *orig, int orig_stride, int16_t *decoded_corner, int decoded_stride, int n, int left, int top, int bottom_left,
			  int top_right, int bl_size, int tr_size, int strong_enabled, const int32_t *preds, const int32_t *pred_bits, int other_bits,
			  double sqrt_lambda, int16_t *adi, int16_t *adi_filtered, int16_t *pred, int pred_stride, int32_t *out, double *best_cost);


/* ------------------------------------------------------------------------------------------------
 * 9. transform-tree consolidation and the luma intra CU driver: the walk of encode_intra_luma (hmr_motion_intra.c:1441-1566) for a
 *    one-level tree (max_intra_tr_depth = 2, rd_mode != RD_FULL).  The TUs themselves are launches of section 7 - the parent TUs of
 *    all CUs in one launch on the parent level's plane, then child 0, 1, 2, 3 of all CUs in four launches on the child level's plane
 *    (a child reads its siblings' reconstruction) - and this kernel is the comparison and the buffer consolidation (:1479-1557):
 *       rule 0 (RD_DIST_ONLY)  dist < parent dist            rule 1 (RD_FAST)  1.25 * (dist + 45 * sum) < parent dist + 45 * parent sum
 *    children win -> levels and reconstruction copied up (synchronize_motion_buffers_luma, :866), cbf of quadrant k = nz_k << 1 | any nz;
 *    parent wins  -> its bottom row and right column copied down (synchronize_reference_buffs, :844), cbf = nz.
 *    No host round trip between search, TUs and decision: a CU's whole luma decision is one ordered chain of launches.
 * ------------------------------------------------------------------------------------------------ */
#define HMR_GPU_TREE_NO_PARENT 0xffffffffu      /* a 64x64 CU has no parent TU (cost preset to INT_MAX, :1402): always consolidated */
typedef struct hmr_gpu_tree_job {
	uint32_t parent;                          /* index of the parent TU in ssd[] / ac_sum[] */
	uint32_t child[4];                        /* indices of the four child TUs, z-order */
	uint32_t par_rec_off, par_rec_stride;     /* the CU in the parent level's plane (decoded_mbs_wnd[depth + 1]) */
	uint32_t chl_rec_off, chl_rec_stride;     /* the CU in the child level's plane (decoded_mbs_wnd[depth + 2]) */
	uint32_t par_lev_off, chl_lev_off;        /* size * size levels each, linear; the children's blocks are consecutive (abs_index order) */
	uint32_t size;                            /* CU size: 8, 16, 32, 64 */
	uint32_t rule;                            /* 0 / 1 above */
} hmr_gpu_tree_job;
typedef struct hmr_gpu_tree_result {
	uint32_t split;                           /* 1 = the four children were kept */
	uint32_t cost, sum;                       /* what the partition node carries afterwards (cost = distortion) */
	uint8_t cbf[4];                           /* cbf byte of the four quadrants (tr_idx = split) */
} hmr_gpu_tree_result;
int hmr_gpu_tree_decide_batch(hmr_gpu_ctx *ctx, const hmr_gpu_tree_job *jobs, int njobs, const uint32_t *ssd, const int32_t *ac_sum, int16_t *recon_base,
			      int16_t *level_base, hmr_gpu_tree_result *out);
/* host-pointer (drop-in) form of the whole luma CU: mode search, parent TU, four child TUs and the consolidation in one submission.
 * nb: 5 x {left, top, bottom_left, top_right, bl_size, tr_size} for the CU and its four quadrants; dec_par / dec_chl: the CU's first sample in the
 * two planes (both hold the neighbours); lev_par / lev_chl: size * size each.
 * out[0] split, [1] = [2] cost, [3] sum, [4..7] cbf, [8] tr_idx, [9..13] ssd of parent + children, [14..18] their sums (slot 0 carries the consolidated
 * figures after a split), [19] mode, [20] its bit count. */
void hmr_gpu_intra_luma_cu(int16_t *orig, int orig_stride, int16_t *dec_par, int dec_par_stride, int16_t *dec_chl, int dec_chl_stride, const int32_t *nb,
			   int strong_enabled, const int32_t *preds, const int32_t *pred_bits, int other_bits, double sqrt_lambda, int16_t *adi, int16_t *adi_filtered,
			   int16_t *pred, int pred_stride, int16_t *lev_par, int16_t *lev_chl, int size, int slice_is_intra, int sign_hiding, int per, int rem, int rule,
			   int32_t *out, double *best_cost);


/* ------------------------------------------------------------------------------------------------
 * 10. chroma half of an intra CU: encode_intra_chroma (hmr_motion_intra_chroma.c:114-471, rd_mode != RD_FULL).
 *     Search: five candidates (planar, vertical, horizontal, DC, DM = the luma mode; an entry equal to the luma mode becomes 34) predicted for U and V
 *     from unfiltered neighbours, cost = dU + (dU + dV) + (uint32)(bits * sqrt_lambda + .5) with bits 1 for DM and 12 otherwise, first minimum wins.
 *     The TUs of the winner are hmr_gpu_itu_job launches of section 7 with is_luma = 0 whose mode comes from this search's result array.
 *     Result: best_mode = prediction mode | coded chroma mode << 8 (36 = DM), bits, cost.
 * ------------------------------------------------------------------------------------------------ */
typedef struct hmr_gpu_chroma_job {
	double sqrt_lambda;                       /* et->rd.sqrt_lambda */
	uint32_t orig_u_off, orig_v_off, orig_stride;
	uint32_t dec_u_off, dec_v_off, dec_stride;   /* corner sample (-1,-1) of the CU in the two planes under reconstruction */
	uint32_t flags;                           /* bits 0 left, 1 top, 2 bottom_left, 3 top_right; bit 8: luma_mode is an index into the luma search results */
	uint32_t sizes;                           /* bl_size | tr_size << 16, in chroma samples */
	uint32_t luma_mode;
	uint32_t reserved;
} hmr_gpu_chroma_job;
/* size = chroma size of the searched block: 4, 8, 16 (a 64x64 CU is searched on its first 32x32 quadrant only, hmr_motion_intra_chroma.c:165-169) */
int hmr_gpu_chroma_search_batch(hmr_gpu_ctx *ctx, const hmr_gpu_chroma_job *jobs, int njobs, int size, const int16_t *orig_base, const int16_t *decoded_base,
				const hmr_gpu_intra_result *luma_modes, hmr_gpu_intra_result *out);
/* host-pointer (drop-in) form of the whole function: search + the U / V TUs of the winner along the luma tree (split = 0: one TU of `size` per component,
 * split = 1: four of size / 2 in z-order; a 4x4 chroma CU is always one TU) in one submission.  size: chroma CU size 4 ... 32; nb: 5 x {left, top,
 * bottom_left, top_right, bl_size, tr_size} in chroma samples for the CU and its quadrants; weight: the chroma distortion weight (:149).
 * out: [0] coded mode, [1] prediction mode, [2] bits, [3] search cost, [4] distortion = sum of (int)(weight * SSD), [5] sum, [6..9] / [10..13] ac sums of
 * the U / V TUs. */
void hmr_gpu_intra_chroma_cu(int16_t *orig_u, int16_t *orig_v, int orig_stride, int16_t *dec_u, int16_t *dec_v, int dec_stride, const int32_t *nb, int luma_mode,
			     int split, double sqrt_lambda, double weight, int16_t *pred_u, int16_t *pred_v, int pred_stride, int16_t *lev_u, int16_t *lev_v, int size,
			     int slice_is_intra, int sign_hiding, int per, int rem, int32_t *out);


/* ------------------------------------------------------------------------------------------------
 * 11. SAO offset derivation (8-bit): sao_derive_offsets + sao_invert_quant_offsets + sao_get_distortion (hmr_sao.c:480-659) for the five types of the
 *     three components of every CTU, straight from the statistics array of hmr_gpu_sao_stats_frame - the part of the SAO decision (sao_derive_mode_new_rdo,
 *     :663) that is a pure function of the statistics.  The rate terms and the off / new / merge comparison read the CABAC state and stay on the host.
 *     stats [ctu][3][5][2][32] int32, lambdas [ctu][3] double (hmr_wpp_sao_ctu, :1415), offsets [ctu][3][5][32], aux [ctu][3][5] (band position; 0 for the
 *     edge types), dist [ctu][3][5] int64; all device pointers.
 * ------------------------------------------------------------------------------------------------ */
int hmr_gpu_sao_offsets_frame(hmr_gpu_ctx *ctx, const int32_t *stats, int n_ctu, const double *lambdas, int32_t *offsets, int32_t *aux, int64_t *dist);
/* host-pointer (drop-in) form for one CTU; lambdas[3] */
void hmr_gpu_sao_offsets_ctu(const int32_t *stats, const double *lambdas, int32_t *offsets, int32_t *aux, int64_t *dist);


/* ------------------------------------------------------------------------------------------------
 * 12. frame encoder: the reference's public API (homer_hevc_enc_api.h:169-174) with the CTU loop of its WPP thread
 *     (wfpp_encoder_thread, hmr_encoder_lib.c:2849-2975: stage the CTU, motion_inter / motion_intra, store, in-loop filters,
 *     entropy coding) running on the device.  One persistent launch walks the picture as the WPP wavefront: a wavefront
 *     per CTU row, row r+1 two CTUs behind row r (:2885-2898); planes, side-info and levels stay resident in HBM.
 *     hmr_gpu_enc_cfg has the layout and field names of HVENC_Cfg (homer_hevc_enc_api.h:138-167), so a caller passes
 *     the struct it already fills for HOMER_enc_control(HOMER_SETCFG).
 *     Built rows: 8-bit 4:2:0, 64x64 CTUs, I / P slices with one reference picture, performance_mode 0-3, max_intra_tr_depth / max_inter_tr_depth up to 4,
 *     rd_mode 0 / 2 and - at fixed QP - rd_mode 1 (RD_FULL: the CABAC bit counter prices the intra decisions); fixed QP and bitrate_mode 1 / 2 (CBR / VBR:
 *     bitrate, vbv_size, vbv_init, frame_rate) - BASELINE configs 0 .. 4.  Rate control and RD_FULL run with one WPP thread (the reference's deterministic
 *     serial mode: the picture one CTU at a time in raster order), with a thread per CTU row, and - rate control - with num_enc_engines > 1 (round 6); RD_FULL with
 *     several engines and RD_FULL under rate control are refused.  Anything else, pictures of more than 128 CTU rows and pictures of more than 192 wavefront steps (CTU columns + 2 x (CTU rows - 1))
 *     make hmr_gpu_enc_create return HMR_GPU_ERR_ARG (hmr_gpu_last_error says why).
 *     wfpp_num_threads = 1: the stream of the reference's single worker thread.  wfpp_num_threads = CTU rows: the stream of its
 *     multi-thread mode with the threads advancing as a synchronous wavefront (pinned by oracle/ref_ctudump.c, HOMER_TURNSTILE);
 *     fewer threads than rows are accepted when 2 x threads >= CTU columns (2160p: 32 threads, the reference's maximum, for 34 rows), others are refused.
 *     Picture grids the compiled reference cannot run are refused too (no stream exists to compare with): two CTU columns x several rows (it crashes),
 *     num_enc_engines > 1 on fewer than nine CTU columns with more than four CTU rows (its engines deadlock), and the two small-grid corners of its
 *     lagged filter pipeline that the frame passes here do not reproduce (enc/enc_host.h make_seq: one CTU column; three columns with four or more rows;
 *     SAO on at most five columns with at least as many rows).
 *     Deblocking, SAO (statistics, decision, syntax, offsets), the CABAC coding of the CTU rows' sub-streams and border padding are tasks of the same launch
 *     (enc/enc_post.h); the host writes parameter sets, slice header, entry points and the NAL escaping.
 * ------------------------------------------------------------------------------------------------ */
typedef struct hmr_gpu_enc_cfg {
	int32_t size, profile, width, height;
	float frame_rate;
	int32_t cu_size, max_pred_partition_depth, max_intra_tr_depth, max_inter_tr_depth, intra_period, gop_size, num_b, num_ref_frames;
	int32_t motion_estimation_precision, qp, chroma_qp_offset, num_enc_engines, wfpp_enable, wfpp_num_threads, sign_hiding, sample_adaptive_offset;
	int32_t bitrate_mode, bitrate, vbv_size, vbv_init, reinit_gop_on_scene_change, rd_mode, performance_mode;
} hmr_gpu_enc_cfg;
typedef struct hmr_gpu_enc hmr_gpu_enc;

/* HOMER_enc_init + HOMER_enc_control(HOMER_SETCFG) */
int hmr_gpu_enc_create(hmr_gpu_ctx *ctx, const hmr_gpu_enc_cfg *cfg, hmr_gpu_enc **out);
/* The same for BATCHES of sequences in the reference's deterministic single-thread order (wfpp_num_threads = 1, num_enc_engines = 1: BASELINE.md's parity mode, the
 * stream of the plain reference without any pinned interleaving): the object's pictures run CTU by CTU in raster order as tasks of the batch launch (section 12b) - one
 * decision in flight per picture, the post-decision tasks beside it - so it takes many pictures per launch to fill the device.  An object made by hmr_gpu_enc_create with
 * one thread, fixed QP and RD_FAST runs the guess / verify / re-encode schedule instead: faster for ONE sequence, not a batch schedule (the batch calls refuse it). */
int hmr_gpu_enc_create_serial_pool(hmr_gpu_ctx *ctx, const hmr_gpu_enc_cfg *cfg, hmr_gpu_enc **out);
/* HOMER_enc_close */
void hmr_gpu_enc_destroy(hmr_gpu_enc *enc);
/* bytes of one per-CTU record of hmr_gpu_enc_frame_ctus (layout of oracle/ref_ctudump.c) */
int hmr_gpu_enc_record_bytes(void);
/* The CTU decisions of one frame (the part of HOMER_enc_encode between slice set-up and the in-loop filters): y / u / v are host
 * 8-bit planes (width x height, width/2 x height/2); image_type as encoder_in_out_t.image_type (0 auto, 3 forced intra);
 * ref_y / ref_u / ref_v, when not NULL, replace the encoder's reference picture (8-bit, unpadded) - used by the parity tests to
 * compare frame by frame against the reference's own pictures; avg_dist < 0 keeps the encoder's own running value.
 * records (host, may be NULL): nctu x hmr_gpu_enc_record_bytes() bytes, one record per CTU. Returns the slice type (1 P, 2 I) or a negative status. */
int hmr_gpu_enc_frame_ctus(hmr_gpu_enc *enc, const uint8_t *y, const uint8_t *u, const uint8_t *v, int image_type, const uint8_t *ref_y, const uint8_t *ref_u,
			   const uint8_t *ref_v, double avg_dist, uint8_t *records);
/* milliseconds the CTU passes of the last frame took on the device (HIP events on the context's stream) */
float hmr_gpu_enc_last_ctu_ms(hmr_gpu_enc *enc);

/* HOMER_enc_encode (homer_hevc_enc_api.h:173, hmr_encoder_lib.c:1655 + encoder_engine_thread :3043-3260): one picture in, one access unit out.
 * CTU decisions, rate control, deblocking, SAO statistics / parameter decision (hmr_sao.c:663-1410) / offsets, the CABAC coding of the CTU rows' sub-streams
 * (hmr_arithmetic_encoding.c, hmr_binary_encoding.c) and border padding run on the device; the host assembles the access unit (hmr_headers.c, hmr_bitstream.c)
 * from the sub-streams.  y / u / v: host 8-bit planes; image_type as encoder_in_out_t.image_type (0 auto, 3 forced intra).  stream receives the
 * Annex-B bytes of the access unit (VPS / SPS / PPS in front of an IDR), *stream_bytes their count; recon (optional) the final picture,
 * 8-bit planar.  Returns the slice type (1 P, 2 I) or a negative status. */
int hmr_gpu_enc_encode(hmr_gpu_enc *enc, const uint8_t *y, const uint8_t *u, const uint8_t *v, int image_type, uint8_t *stream, long cap, long *stream_bytes,
		       uint8_t *recon);
/* the same with the source picture already resident in HBM: load_source converts and keeps a picture in slot `slot`, encode_source encodes it */
int hmr_gpu_enc_load_source(hmr_gpu_enc *enc, int slot, const uint8_t *y, const uint8_t *u, const uint8_t *v);
int hmr_gpu_enc_encode_source(hmr_gpu_enc *enc, int slot, int image_type, uint8_t *stream, long cap, long *stream_bytes, uint8_t *recon);
/* one frame of each of n sequences with ONE launch for all their CTU stages: encs[i] encodes its resident picture slots[i] (image_types may be NULL: automatic)
 * into streams[i] (capacity caps[i], size stream_bytes[i]).  The encoders use the row-per-thread schedule (wfpp_num_threads > 1) and the same device; the access
 * units are those hmr_gpu_enc_encode_source gives one by one.  The launch is a pool of persistent row workers (four per CU; as many as the pictures can keep busy)
 * that claim CTUs of any of the n pictures whose wavefront step is open (k_encode_pool); n is at most 512, a few hundred pictures' worth of CTU rows saturate the pool
 * (120 at 1080p; a launch costs about 110 ms of ramps on top of 1.7 ms per 1080p picture, so more pictures per launch amortise it: 256 -> 512 is +10 %).  A worker never waits for a CTU that is not already running, so the launch does not depend on all its
 * workgroups being resident; a watchdog (HENC_WATCHDOG_S seconds, fractions allowed, 120 by default) makes a launch in which a worker has found nothing to do - no CTU
 * to decide, no post-decision task - for that long SINCE IT LAST DID return HMR_GPU_ERR_HIP instead of hanging. */
int hmr_gpu_enc_encode_batch(hmr_gpu_enc **encs, int n, const int *slots, const int *image_types, uint8_t **streams, const long *caps, long *stream_bytes);
/* the same, pipelined: call k launches the frames slots[] and delivers the access units of call k - 1's frames (stream_bytes[i] = 0 on the first call), whose download
 * and entropy coding run while the device is busy with call k's CTU stage - a frame's successor needs its reconstruction and its distortion statistic, not its bytes
 * (the reference's interface is asynchronous in the same way: HOMER_enc_encode queues a picture, HOMER_enc_get_coded_frame, hmr_encoder_lib.c:2997, takes coded frames
 * from the output queue later).  slots == NULL: deliver the outstanding
 * access units only (flush).  encs / n stay the same from call to call until the flush; an encoder with an access unit outstanding is refused by the other encode calls. */
int hmr_gpu_enc_encode_batch_pipelined(hmr_gpu_enc **encs, int n, const int *slots, const int *image_types, uint8_t **streams, const long *caps, long *stream_bytes);
/* the last frame: passes of the CTU schedule, CTU encodes (>= the number of CTUs), device milliseconds of the CTU passes and of the whole frame */
int hmr_gpu_enc_last_stats(hmr_gpu_enc *enc, int *passes, int *ctu_encodes, float *ctu_ms, float *frame_ms);
/* which kernel ran the last pool launch this encoder led (alone, or as the first encoder of a batch call) - 0: the latency kernel (at most one worker per compute
 * unit), 1: the throughput kernel, whose decision walk is compiled without full RDO (no RD_FULL picture in the launch), 2: the generic kernel (a launch with an
 * RD_FULL picture); -1: none yet */
int hmr_gpu_enc_last_pool_kernel(hmr_gpu_enc *enc);
/* The one place where byte identity with the reference is not guaranteed, counted: a merge candidate whose vector points outside the padded reference picture
 * (more than 80 samples beyond the frame) is evaluated by the reference on whatever its thread's prediction window holds (check_rd_cost_merge_2nx2n leaves out
 * the motion compensation and nothing else, hmr_motion_inter.c:3651).  The window travels with the thread here too (the stream is the
 * reference's when its content came from block writes), but the reference's SSE predictors also leave samples outside the blocks they predict (e.g. 255s right of
 * a 4 x 4 angular chroma block), which are not reproduced.  *last_picture: such evaluations in the last picture encoded through this object (-1: none encoded
 * yet; counted in both thread orders), *all_pictures: since the object was created.  0 = the quirk did not occur (every clip of bench.py; 12 of about 3000 random fuzz cases
 * had it, one of them differs: profiles/r04_encoder_fuzz.md).  Either pointer may be NULL. */
int hmr_gpu_enc_stale_predictions(hmr_gpu_enc *enc, long *last_picture, long *all_pictures);
/* profiling build (-DHENC_PROFILE): per-row phase timers, [ctu rows][12] */
int hmr_gpu_enc_profile(hmr_gpu_enc *enc, unsigned long long *out, int reset);
/* profiling build, row-per-thread schedule: per CTU four 100 MHz timestamps {wait start, encode start, first use of the intra share (0: none), end}, [ctus][4] */
int hmr_gpu_enc_timeline(hmr_gpu_enc *enc, unsigned long long *out);

/* ------------------------------------------------------------------------------------------------
 * 12b. Engines: hvenc_enc_t.num_encoder_engines / encoder_engine_thread (hmr_encoder_lib.c:3043-3330; hmr_private.h:1232)
 *     hmr_gpu_enc_cfg.num_enc_engines = E > 1 (row-per-thread schedule; with wfpp_num_threads = 1 only as ONE object that holds all engines, hmr_gpu_enc_create,
 *     which then runs the picture CTU by CTU on the pool's raster schedule) gives the stream of the reference's frame pipeline in the
 *     interleaving oracle/ref_ctudump.c's engine turnstile pins on it: frame n is encoded on the complete reconstruction of frame
 *     n - 1, starts from the avg_dist frame n - E left behind and works on the persistent state of engine n mod E.
 *     hmr_gpu_enc_create keeps all E engines in one object.  hmr_gpu_enc_create_engine makes ONE engine (index k of E): it is given
 *     only the frames k, k + E, ... and, before each of them except frame 0, the hand-over of the engine before it -
 *     hmr_gpu_enc_export_reference on that engine after its frame, hmr_gpu_enc_import_reference here: the reconstructed picture
 *     (three padded int16 planes in DEVICE memory, hmr_gpu_enc_reference_elems(enc, comp) elements each, e.g. buffers an RCCL
 *     send / recv moves between GPUs) and hmr_gpu_enc_state_bytes() bytes of frame-to-frame scalars (host memory).
 * ------------------------------------------------------------------------------------------------ */
int hmr_gpu_enc_create_engine(hmr_gpu_ctx *ctx, const hmr_gpu_enc_cfg *cfg, int engine_index, hmr_gpu_enc **out);
int hmr_gpu_enc_state_bytes(void);
long hmr_gpu_enc_reference_elems(hmr_gpu_enc *enc, int comp);
int hmr_gpu_enc_export_reference(hmr_gpu_enc *enc, int16_t *dev_y, int16_t *dev_u, int16_t *dev_v, void *state);
int hmr_gpu_enc_import_reference(hmr_gpu_enc *enc, const int16_t *dev_y, const int16_t *dev_u, const int16_t *dev_v, const void *state);
/* The hand-over of n engines at once with the picture as it travels between GPUs: 8-bit samples without margins (hmr_gpu_enc_reference_bytes: width x height
 * luma, then the two chroma planes; 3.1 MB at 1080p against 6.6 MB of padded int16 planes), picture i at dev_rows + i * pitch in DEVICE memory; the importer
 * widens the samples and rebuilds the margins (reference_picture_border_padding_ctu, hmr_encoder_lib.c:1723).  states: n x hmr_gpu_enc_state_bytes() bytes (host). */
long hmr_gpu_enc_reference_bytes(hmr_gpu_enc *enc);
/* 12c. Overlapping engines on one GPU.  The reference's engine k + 1 follows engine k's frame at the distance of the search window and the filter lag, CTU row by CTU row
 * (hmr_encoder_lib.c:2393-2403 the lag arithmetic, :2440-2445 the per-CTU SEM_POST of synchro_signal[1], :3154-3211 the frame hand-out).  hmr_gpu_enc_encode_chain encodes
 * the frames slots[0 .. n - 1] (n <= num_enc_engines; more with twins, below) of ONE sequence on its engine objects encs[0 .. n - 1] (in coding order; prev = the object that encoded the frame
 * before, NULL at the sequence start) in one launch of the CTU kernel: frame j predicts from the final picture of frame j - 1 where it lies (no copy) and from its phase
 * planes, which the same launch produces CTU by CTU; a wavefront step of frame j starts when the part of that picture its vectors can reach is ready.  Same streams as frame
 * by frame (the engine turnstile's interleaving, oracle/ref_ctudump.c).  Returns HMR_GPU_ERR_ARG when two frames of the chain both detect a scene change (sequentially the
 * first switches the detection off for the second): repeat those frames one by one.  A call that is refused while its frames are being set up (wrong engine for a frame, a P
 * frame without the object that holds the picture before it, an I frame too early in the chain) leaves every object as it found it.  Chains of more than one frame are refused
 * under rate control and with rd_mode RD_FULL: both read entropy-coder state of the frame before (hmr_rate_control.c:266-282, the coder objects' context states), which a
 * chain's frames, started from a predicted state, do not have - encode those sequences frame by frame.
 * More frames than engines (n up to 32): the reference's engine k takes frame t + num_enc_engines when its frame t is finished.  hmr_gpu_enc_create_engine_twin makes
 * another object for the same engine - it shares the engine's persistent state (CTU records, the WPP threads' mode buffers) with `of` and has its own pictures, filter state
 * and sub-stream buffers; encs[j] for j >= num_enc_engines has to be a twin of encs[j - num_enc_engines] (or the other way round).  The launch then starts an engine's next
 * frame when its previous one is finished and hands on the average distortion it leaves (hmr_encoder_lib.c:3217-3262) inside the launch; the engines never idle between the
 * frames of a call.  An I frame inside the sequence must be among the last num_enc_engines frames of its call (it hands on the value of the frame before it).  Destroy the
 * twins before the object they were made from. */
int hmr_gpu_enc_create_engine_twin(hmr_gpu_ctx *ctx, hmr_gpu_enc *of, hmr_gpu_enc **out);
int hmr_gpu_enc_encode_chain(hmr_gpu_enc **encs, int n, hmr_gpu_enc *prev, const int *slots, const int *image_types, uint8_t **streams, const long *caps, long *stream_bytes);
int hmr_gpu_enc_export_references8(hmr_gpu_enc **encs, int n, uint8_t *dev_rows, long pitch, void *states);
int hmr_gpu_enc_import_references8(hmr_gpu_enc **encs, int n, const uint8_t *dev_rows, long pitch, const void *states);

/* ------------------------------------------------------------------------------------------------
 * 12d. Pictures in device memory (no counterpart in the reference, whose pictures arrive in host memory)
 *     A decoder, a renderer or a tensor library leaves its pictures on the GPU.  hmr_gpu_enc_load_sources_device converts n of them (1 .. 512) into picture slots of
 *     their encoders with ONE launch of a bandwidth-bound kernel (k_ingest, picture_io.hip) and no host synchronisation; the slots are what hmr_gpu_enc_load_source makes of the
 *     same samples, so every encode call of section 12 takes them.  8-bit 4:2:0 as I420 (three planes) or NV12 (luma plane, plane of interleaved U, V pairs); any base
 *     address, every plane with a byte pitch of its own (at least a row's bytes: width for luma and for NV12's pairs, width / 2 for I420 chroma).  Only the bytes of the
 *     rows are read - [plane + y * pitch, plane + y * pitch + row bytes) - so the last row may end with the caller's allocation.
 *     producer_stream is the hipStream_t (NULL: the null stream, treated like any other) on which the caller's work that WRITES the pictures is queued, e.g. torch's
 *     current stream.  The library records an event on it and the ingest waits for that event; behind the ingest it records an event of its own and lets
 *     producer_stream wait for it.  So the pictures need not be finished when the call is made, and whatever the caller queues on producer_stream after the call
 *     returns - overwriting the pictures, an allocator handing their memory on - runs after the library has read them.  The host waits for nothing in either direction
 *     (a slot that does not exist yet is allocated first, which synchronises the encoder's stream once, as hmr_gpu_enc_load_source does).
 *     Towards the encode calls: the ingest runs on the first encoder's stream and the streams of all the call's encoders are made to wait for it, so a following
 *     hmr_gpu_enc_encode_source, _encode_batch, _encode_batch_pipelined or _encode_chain of any of them sees the pictures, again without the host waiting.  Loading a slot
 *     that an earlier encode call used is ORDERED behind that call, never refused: every encode call of section 12 - the pipelined one too, of which only the download and
 *     the coding of the access units stay outstanding - returns after its launch has read the source pictures for the last time.  (As everywhere in this interface, calls
 *     on one encoder are made from one host thread at a time.)
 *     Refused with HMR_GPU_ERR_ARG before anything is queued: n outside 1 .. 512, a NULL encoder, a slot outside 0 .. 4096, encoders on different devices, the same
 *     (encoder, slot) twice in a call, a descriptor hmr_gpu_picture_check refuses for the encoder's picture size, a plane pointer that hipPointerGetAttributes does not
 *     report as device memory of the encoders' device.
 * ------------------------------------------------------------------------------------------------ */
enum { HMR_GPU_PIC_I420 = 0, HMR_GPU_PIC_NV12 = 1 };
typedef struct hmr_gpu_picture {
	int32_t format, reserved;      /* HMR_GPU_PIC_*; 0 */
	const uint8_t *plane[3];       /* device pointers; NV12: plane[1] = UV pairs, plane[2] = NULL */
	int64_t pitch[3];              /* bytes from row to row */
} hmr_gpu_picture;
/* pure host check of a descriptor against a picture size: no device, no context.  HMR_GPU_OK, or HMR_GPU_ERR_ARG with the field named by hmr_gpu_last_error: NULL
 * descriptor, unknown format, non-zero reserved, odd or non-positive width / height, a missing plane pointer, plane[2] given with NV12, a negative pitch, a pitch
 * smaller than a row's bytes. */
int hmr_gpu_picture_check(const hmr_gpu_picture *pic, int width, int height);
int hmr_gpu_enc_load_source_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_picture *pic, void *producer_stream);
int hmr_gpu_enc_load_sources_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_picture *pics, void *producer_stream);

/* ------------------------------------------------------------------------------------------------
 * 12e. Reconstructed pictures and their quality, left in device memory: homer_psnr (hmr_metics.c:53-105, called for every frame at hmr_encoder_lib.c:3350)
 *     The mirror image of 12d.  hmr_gpu_enc_export_pictures_device hands the pictures of n encoders (1 .. 512) to the caller as 8-bit 4:2:0 in DEVICE memory and / or
 *     leaves the exact sums of squared differences between each picture and a picture slot of its encoder in device memory, with ONE launch of a bandwidth-bound
 *     kernel (k_egress, picture_io.hip) and no host synchronisation.
 *     "The picture" of an encoder is the final picture (after deblocking and SAO: what the next frame predicts from, what a decoder reconstructs) of the frame its last
 *     encode call encoded: hmr_gpu_enc_encode, _encode_source, _encode_batch, _encode_batch_pipelined (the picture of the frames launched by THAT call - the access
 *     unit arrives a call later, the picture does not; an encoder with an access unit outstanding is accepted here) and _encode_chain (every object of the chain holds
 *     its own frame's picture, twins included).  An encoder that has not encoded anything yet is refused.
 *     pics (or NULL: no pictures): n descriptors of OUTPUT pictures - hmr_gpu_picture as in 12d, but the call WRITES through the plane pointers (the const of the type
 *     describes the ingest).  I420 or NV12, any base address, every plane with a byte pitch of its own, at least a row's bytes.  Only the bytes of the rows are written
 *     - [plane + y * pitch, plane + y * pitch + row bytes) - so the picture may be a view into something larger and its last row may end with the caller's allocation.
 *     slots (or NULL: no sums) with dev_ssd (device memory, n x 3 values; NULL exactly when slots is NULL): dev_ssd[3 * i + c] = the sum over the width x height
 *     (chroma: width / 2 x height / 2) samples of (slot picture - final picture)^2 of plane c, exact, against whatever picture slot slots[i] of encs[i] holds when the
 *     launch runs.  Normally that is the slot the frame was encoded from, and then the caller must not have loaded another picture into it in between; any loaded slot
 *     is legal and gives the distance to that picture.  A sum does not fit 32 bits (255^2 x 3840 x 2160 = 5.4e11).  hmr_gpu_psnr turns three sums into homer_psnr's
 *     three values: 10 * log10(255 * 255 * samples / sum) in double, the chroma planes with (width / 2) * (height / 2) samples, and 99.99 where the sum is 0.  It is pure
 *     host code: no device, no context.
 *     consumer_stream is the hipStream_t (NULL: the null stream) on which the caller's work that uses the output memory and dev_ssd is queued, e.g. torch's current
 *     stream.  The library records an event on it and the egress waits for that event (the consumer may still be using the memory); the egress is also queued behind
 *     whatever the encoders' streams hold (the launch that writes the picture, a load into the slot).  Behind the egress the library records an event that
 *     consumer_stream and the streams of all the call's encoders wait for: what the caller queues on consumer_stream after the call sees the pictures and the sums, a
 *     later encode call (which rewrites the final picture two frames on) and a later load into the slot run after the egress has read them.  The host waits for
 *     nothing in either direction.
 *     Refused with HMR_GPU_ERR_ARG and a text (hmr_gpu_last_error) before anything is queued, every encoder left working: n outside 1 .. 512, a NULL encoder, encoders
 *     on different devices, both pics and slots NULL, slots without dev_ssd or the reverse, a slot that does not exist, an encoder without an encoded picture, a
 *     descriptor hmr_gpu_picture_check refuses for the encoder's picture size, an output plane or dev_ssd that hipPointerGetAttributes does not report as device memory
 *     of the encoders' device.  hmr_gpu_psnr: NULL arguments, an odd or non-positive width or height.
 * ------------------------------------------------------------------------------------------------ */
int hmr_gpu_enc_export_pictures_device(hmr_gpu_enc **encs, int n, const hmr_gpu_picture *pics, const int *slots, uint64_t *dev_ssd, void *consumer_stream);
/* one encoder; slot -1: no sums (dev_ssd NULL) */
int hmr_gpu_enc_export_picture_device(hmr_gpu_enc *enc, const hmr_gpu_picture *pic, int slot, uint64_t *dev_ssd, void *consumer_stream);
int hmr_gpu_psnr(const uint64_t ssd[3], int width, int height, double psnr[3]);

/* ------------------------------------------------------------------------------------------------
 * 12f. RGB pictures in device memory: colour conversion inside the ingest (no counterpart in the reference)
 *     A renderer leaves packed RGBA, a tensor library a [3, H, W] tensor, usually float in 0 .. 1.  hmr_gpu_enc_load_sources_rgb_device converts n such pictures
 *     (1 .. 512; formats, matrices and ranges may be mixed within a call) to 8-bit 4:2:0 Y'CbCr and into picture slots of their encoders with ONE launch of a
 *     bandwidth-bound kernel (k_ingest_rgb, picture_io.hip): every source sample is read once, nothing is written but the slot.  It carries the contract of 12d word
 *     for word: the launch runs on the first encoder's stream behind what producer_stream holds now, producer_stream and the other encoders' streams go on behind it,
 *     the host waits for nothing (but for a slot that has to be allocated first); only the bytes of the rows are read, nothing outside width x height of the slot is
 *     written; a slot filled this way is indistinguishable, to every encode call, from one filled by hmr_gpu_enc_load_sources_device with the converted I420 picture.
 *     Refused as in 12d, plus whatever hmr_gpu_rgb_picture_check refuses.
 *     The arithmetic is defined in integers, so that a caller can reproduce every sample (homerhevc_amd/csrc/rgb_yuv.h holds it once, for the kernel and the host):
 *       inputs: 8-bit R, G, B.  A float sample x (binary16 widened exactly to binary32) becomes q = x > 0 ? (x < 1 ? x : 1) : 0 (NaN: 0), v = (int)rintf(q * 255.0f) -
 *         one binary32 product, round half to even, what np.rint(np.float32(q) * np.float32(255)) gives.
 *       luma, per pixel:     Y = ((Yr R + Yg G + Yb B + 32768) >> 16) + yoff
 *       chroma, per 2 x 2 block, SR, SG, SB the sums of its four pixels (the block's average, sited at its centre):
 *                            U = clamp(((Ur SR + Ug SG + Ub SB + 131072) >> 18) + 128, 0, 255), V likewise; >> is an arithmetic shift of a 32-bit signed value
 *       matrix, range     Yr, Yg, Yb            Ur, Ug, Ub               Vr, Vg, Vb              yoff
 *       BT.601 limited    16829, 33039, 6416    -9714, -19070, 28784     28784, -24103, -4681    16
 *       BT.601 full       19595, 38470, 7471    -11058, -21710, 32768    32768, -27439, -5329    0
 *       BT.709 limited    11966, 40254, 4064    -6596, -22188, 28784     28784, -26145, -2639    16
 *       BT.709 full       13933, 46871, 4732    -7509, -25259, 32768     32768, -29763, -3005    0
 *     Every output is within 0.51 of the real-valued BT formula; grey gives U = V = 128 at every level; limited-range luma stays in 16 .. 235 and chroma in 16 .. 240.
 *     The stream does NOT say which matrix or range was used: the parameter sets stay byte-identical to the reference's, which writes no colour description into the VUI.
 *     Whoever decodes the stream has to be told by other means.  (Out of scope as well: other chroma sitings, 10-bit RGB - 10-bit Y'CbCr: section 12k -, bfloat16, alpha - a fourth byte is ignored.)
 *     hmr_gpu_rgb_picture_check: pure host, like hmr_gpu_picture_check; names the field.  Refused: NULL descriptor, unknown format, matrix, full_range outside 0 / 1,
 *     non-zero reserved, odd or non-positive width / height; PACKED8: pixel_bytes not 3 or 4, an offset outside 0 .. pixel_bytes - 1 or repeated, plane[0] NULL,
 *     plane[1] or plane[2] given; planar: pixel_bytes or an offset not 0, a NULL plane; a negative pitch or one below a row's bytes (width x pixel_bytes, width x
 *     element size); float formats: a plane or a pitch that is not a multiple of the element size.
 *     hmr_gpu_rgb_convert_host: the same arithmetic in a plain loop over HOST memory - the descriptor's planes are host pointers here - into tightly packed I420 planes
 *     (y: width x height, u, v: width / 2 x height / 2).  No device, no context.  A utility in the spirit of hmr_gpu_psnr, e.g. to compute quality against the
 *     samples that were encoded; it is not a fallback for encoding.
 *     hmr_gpu_enc_export_sources_device writes what picture slots hold - the pictures the encoders were given, after conversion - as 8-bit I420 or NV12 into the
 *     caller's DEVICE pictures (descriptors as in 12e: written through the plane pointers), ONE launch of k_egress on the first encoder's stream.  It is ordered behind
 *     consumer_stream and behind the encoders' own streams (a load into the slot); consumer_stream and those streams go on behind it; the host waits for nothing.
 *     Refused: n outside 1 .. 512, a NULL encoder, encoders on different devices, a slot that does not exist, a descriptor hmr_gpu_picture_check refuses, an output
 *     plane that is not device memory of the encoders' device.
 * ------------------------------------------------------------------------------------------------ */
enum { HMR_GPU_RGB_PACKED8 = 0, HMR_GPU_RGB_PLANAR8 = 1, HMR_GPU_RGB_PLANAR_F16 = 2, HMR_GPU_RGB_PLANAR_F32 = 3 };
enum { HMR_GPU_MATRIX_BT601 = 0, HMR_GPU_MATRIX_BT709 = 1 };
typedef struct hmr_gpu_rgb_picture {
	int32_t format, matrix, full_range, reserved;   /* HMR_GPU_RGB_*; HMR_GPU_MATRIX_*; 0: limited range, 1: full range; 0 */
	int32_t pixel_bytes;           /* PACKED8: 3 or 4; otherwise 0 */
	int32_t offset[3];             /* PACKED8: byte of R, G, B inside a pixel, distinct, < pixel_bytes (RGB, BGR, RGBA, BGRA, ARGB ...; a fourth byte is ignored); otherwise 0 */
	const void *plane[3];          /* PACKED8: plane[0] only, the others NULL; planar: R, G, B */
	int64_t pitch[3];              /* bytes from row to row, >= a row's bytes; float formats: a multiple of the element size, planes aligned to it */
} hmr_gpu_rgb_picture;
int hmr_gpu_rgb_picture_check(const hmr_gpu_rgb_picture *pic, int width, int height);
int hmr_gpu_rgb_convert_host(const hmr_gpu_rgb_picture *pic, int width, int height, uint8_t *y, uint8_t *u, uint8_t *v);
int hmr_gpu_enc_load_source_rgb_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_rgb_picture *pic, void *producer_stream);
int hmr_gpu_enc_load_sources_rgb_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_rgb_picture *pics, void *producer_stream);
int hmr_gpu_enc_export_source_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_picture *out, void *consumer_stream);
int hmr_gpu_enc_export_sources_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_picture *outs, void *consumer_stream);

/* ------------------------------------------------------------------------------------------------
 * 12g. A resolution ladder from pictures in device memory: downscaling inside the ingest (no counterpart in the reference, which has no scaler)
 *     One decoded or rendered picture is to be encoded at several sizes.  hmr_gpu_enc_load_sources_scaled_device fills picture slots of n encoders (1 .. 512) from
 *     8-bit 4:2:0 pictures that are LARGER than (or as large as) the encoders' pictures, area-averaged down to each encoder's size, with ONE launch of a kernel
 *     (k_downscale, picture_io.hip) that reads every source picture once per entry.  The same source picture may appear in any number of entries of a call - that is
 *     the ladder; sizes, ratios and formats may be mixed freely within a call; an entry whose source has the encoder's size is legal and gives exactly what
 *     hmr_gpu_enc_load_sources_device gives.  The source is I420 or NV12 at any base address and pitch, so a crop is just a view.
 *     It carries the contract of 12d word for word: the launch runs on the first encoder's stream behind what producer_stream holds now, producer_stream and the
 *     other encoders' streams go on behind it, the host waits for nothing (but for a slot that has to be allocated first); only the bytes of the source's rows are
 *     read, nothing outside width x height of the slot is written; a slot filled this way is indistinguishable, to every encode call, from one filled by
 *     hmr_gpu_enc_load_sources_device with the host-scaled I420 picture.  hmr_gpu_enc_export_sources_device (12f) returns what the slot holds.
 *     Refused as in 12d, with the descriptor checked against the SOURCE's size (hmr_gpu_scaled_picture.width, .height), plus whatever hmr_gpu_scale_check refuses
 *     for (source size -> encoder size).
 *     The arithmetic is defined in integers, so that a caller can reproduce every sample (homerhevc_amd/csrc/scale_area.h holds it once, for the kernel and the host).
 *     Area averaging, downscaling only.  Every plane is scaled on its own: luma Ws x Hs -> Wd x Hd, each chroma plane Ws/2 x Hs/2 -> Wd/2 x Hd/2, which keeps the
 *     4:2:0 siting.  Per axis with source length S and destination length D:
 *       g = gcd(S, D), s = S / g, d = D / g.  A source sample is d units wide, an output sample s units wide.
 *       output x covers [x s, (x + 1) s); source sample i covers [i d, (i + 1) d)
 *       tap weight w(x, i) = min((x + 1) s, (i + 1) d) - max(x s, i d) where that is positive; the weights of one output sum to s; at most ceil(S / D) + 1 taps
 *     and, with ONE rounding and no intermediate rounding,
 *       out(x, y) = (sum_j sum_i wy(y, j) wx(x, i) src(i, j) + (sx sy >> 1)) / (sx sy)
 *     in unsigned 32-bit arithmetic; the division is an unsigned integer division.  The order of the passes therefore cannot change a bit.
 *     Equal sizes give the identity; 2 : 1 gives (a + b + c + d + 2) >> 2; every output is within 0.5 of the real-valued area average.  sx sy is 9 for
 *     1920 x 1080 -> 1280 x 720, 540 for 1920 x 1080 -> 416 x 240 and 21945 for 330 x 266 -> 328 x 264.
 *     hmr_gpu_scale_check: pure host - no device, no context; names the field.  Refused: a non-positive or odd value among the four; dst > src on an axis (no
 *     upscaling: area averaging degenerates to nearest neighbour there); src > 8 dst on an axis; a source axis above 65536; sx sy 255 + (sx sy >> 1) >= 2^32 (luma
 *     and chroma have the same sx, sy) - every even size up to 8192 x 4320 passes.
 *     hmr_gpu_scale_host: the same arithmetic in a plain loop over HOST memory - the descriptor's planes are host pointers here - into tightly packed I420 planes
 *     (y: dst_w x dst_h; u, v: dst_w / 2 x dst_h / 2).  No device, no context.  A utility in the spirit of hmr_gpu_rgb_convert_host; it is not a fallback for encoding.
 *     It refuses what hmr_gpu_picture_check and hmr_gpu_scale_check refuse, except that it takes any ratio: the bound of 8 is the kernel's, not the arithmetic's.
 *     RGB sources: section 12j, which fills a slot with exactly this section's average of the picture 12f makes, in one launch and without that picture in memory.
 * ------------------------------------------------------------------------------------------------ */
typedef struct hmr_gpu_scaled_picture {
	hmr_gpu_picture pic;           /* the SOURCE picture, as in 12d */
	int32_t width, height;         /* the SOURCE's size */
} hmr_gpu_scaled_picture;
int hmr_gpu_scale_check(int src_w, int src_h, int dst_w, int dst_h);
int hmr_gpu_enc_load_sources_scaled_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_scaled_picture *pics, void *producer_stream);
int hmr_gpu_enc_load_source_scaled_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_scaled_picture *pic, void *producer_stream);
int hmr_gpu_scale_host(const hmr_gpu_scaled_picture *pic, int dst_w, int dst_h, uint8_t *y, uint8_t *u, uint8_t *v);

/* ------------------------------------------------------------------------------------------------
 * 12h. SSIM of the reconstructed pictures, left in device memory (no counterpart in the reference, whose only metric is homer_psnr)
 *     PSNR ranks the rungs of a ladder and quantisers that blur differently badly; the metric expected beside it is SSIM.  hmr_gpu_enc_ssim_device leaves, for n
 *     encoders (1 .. 512), the exact sums of a fixed-point SSIM value over all windows of each plane between the encoder's final picture and a picture slot, with ONE
 *     launch of a kernel (k_ssim, picture_io.hip) that reads both pictures' int16 planes once (plus a tile's rim) and writes nothing but the sums; no host
 *     synchronisation.  "The picture" of an encoder is 12e's: the final picture of the frame its last encode call encoded - single, batch, pipelined batch (an
 *     encoder with an access unit outstanding is accepted) or chain (every object holds its own frame's picture); the slot is whatever slots[i] of encs[i] holds
 *     when the launch runs - normally the slot the frame was encoded from; any loaded slot is legal.
 *     The arithmetic is defined in integers, so that a caller can reproduce every sum (homerhevc_amd/csrc/ssim_window.h holds it once, for the kernel and the host).
 *     Every plane on its own: luma width x height, each chroma plane width / 2 x height / 2; a = the slot's samples, b = the final picture's.  Every size the frame
 *     encoder accepts is a multiple of 8, so a w x h plane is an exact grid of bw x bh = (w / 4) x (h / 4) BLOCKS of 4 x 4 samples.
 *       block sums, over a block's 16 samples:   s1 = sum a    s2 = sum b    ss = sum (a a + b b)    s12 = sum a b
 *       windows: every 2 x 2 group of adjacent blocks - 8 x 8 samples; neighbouring windows overlap by one block; (bw - 1) (bh - 1) windows a plane.
 *         S1, S2, SS, S12 = the sums of the four blocks' sums
 *       per window, in exact integers, C1 = 416 = floor((0.01 255)^2 64 + 0.5), C2 = 235963 = floor((0.03 255)^2 64 63 + 0.5) (the usual 8 x 8 block-SSIM constants):
 *         var = 64 SS - S1 S1 - S2 S2        cov = 64 S12 - S1 S2
 *         N = (2 S1 S2 + C1) (2 cov + C2)    D = (S1 S1 + S2 S2 + C1) (var + C2)
 *         q = floor(2^30 N / D), the floor towards minus infinity (N may be negative: a window of a picture against its inverse)
 *       per plane:  sum[c] = the sum of q over the plane's windows, a signed 64-bit integer - exact in any order of addition.  It does not fit 32 bits: a 2160p luma
 *         plane of identical pictures gives 2^30 x 959 x 539 = 5.5e14.
 *       mean SSIM of plane c = sum[c] / (2^30 windows[c]): hmr_gpu_ssim, one double division on the host.
 *     Bounds: 0 < D < 2^57, |N| <= D, so -2^30 <= q <= 2^30, and q = 2^30 exactly when the window's samples are equal in a and b (ssim_window.h derives them).
 *     2^30 N does not fit 64 bits; ssim_window.h says how the exact quotient is reached in 64-bit arithmetic - the result is the formula's, bit for bit.
 *     What is read: the h rows (chroma: h / 2) of each int16 plane, [row, row + stride) of each - a plane with an odd number of block columns has a last 16-byte span
 *     whose second half lies beyond the row's w samples, inside the row's stride (strides are multiples of 8 elements); those values are ignored.
 *     dev_ssim (device memory, n x 3 values): dev_ssim[3 * i + c] = sum[c] of encs[i].
 *     consumer_stream: as in 12e, word for word.  The launch runs on the first encoder's stream behind an event recorded on consumer_stream (the consumer may still be
 *     using dev_ssim), behind the launches that wrote the final pictures and behind whatever the encoders' streams hold (a load into the slot); the sums are zeroed on
 *     that stream in front of the launch.  Behind the launch the library records an event that consumer_stream and the streams of all the call's encoders wait for:
 *     what the caller queues on consumer_stream after the call sees the sums, a later encode call and a later load into the slot run after the kernel has read the
 *     pictures.  The host waits for nothing in either direction.
 *     Refused with HMR_GPU_ERR_ARG and a text (hmr_gpu_last_error) before anything is queued, every encoder left working: n outside 1 .. 512, NULL encs, slots or
 *     dev_ssim, a NULL encoder, encoders on different devices, a slot that does not exist, an encoder without an encoded picture, a picture below 16 samples in width
 *     or height (a chroma plane with fewer than two block rows or columns has no window), dev_ssim that hipPointerGetAttributes does not report as device memory of
 *     the encoders' device.
 *     hmr_gpu_ssim: sums[c] / (2^30 windows[c]) for the three planes of a width x height picture, in double: both operands are exact below 2^53, so the result is the
 *     correctly rounded quotient.  Pure host code: no device, no context.  Refused: NULL arguments, a width or height that is not a positive multiple of 8 or is below
 *     16, a sum outside +- 2^30 windows.
 *     hmr_gpu_ssim_host: the same arithmetic in plain nested loops over two 8-bit pictures in HOST memory - the descriptors' planes are host pointers here; I420 or
 *     NV12 (the two may differ), any pitch - into sums[3].  No device, no context.  A utility in the spirit of hmr_gpu_scale_host.  It refuses what
 *     hmr_gpu_picture_check refuses for either picture, the sizes hmr_gpu_ssim refuses, and NULL sums.
 *     Out of scope: a call on arbitrary 8-bit device pictures, MS-SSIM, Gaussian windows, one figure for Y, U and V together.
 * ------------------------------------------------------------------------------------------------ */
int hmr_gpu_enc_ssim_device(hmr_gpu_enc **encs, int n, const int *slots, int64_t *dev_ssim, void *consumer_stream);
int hmr_gpu_enc_ssim_one_device(hmr_gpu_enc *enc, int slot, int64_t *dev_ssim, void *consumer_stream);
int hmr_gpu_ssim(const int64_t sums[3], int width, int height, double ssim[3]);
int hmr_gpu_ssim_host(const hmr_gpu_picture *a, const hmr_gpu_picture *b, int width, int height, int64_t sums[3]);

/* ------------------------------------------------------------------------------------------------
 * 12i. Reconstructed pictures as RGB, left in device memory: colour conversion inside the egress (no counterpart in the reference)
 *     The mirror image of 12f, as 12e mirrors 12d.  hmr_gpu_enc_export_pictures_rgb_device hands pictures of n encoders (1 .. 512; sizes, forms, matrices and ranges may
 *     be mixed within a call) to the caller as RGB in DEVICE memory and / or leaves the exact sums of squared differences between each picture's 8-bit R, G, B values
 *     and an RGB picture of the caller's - the frame that was actually supplied - with ONE launch of a bandwidth-bound kernel (k_egress_rgb, picture_io.hip) and no host
 *     synchronisation.  Nothing on the encode path is touched: every stream stays byte-identical.
 *     which[i]: -1: the encoder's final picture, exactly "the picture" of 12e (an encoder without an encoded picture is refused); >= 0: whatever picture slot which[i]
 *     of encs[i] holds when the launch runs - the encoded source seen as RGB; this needs no prior encode.
 *     outs (or NULL: no pictures): n descriptors of OUTPUT pictures - hmr_gpu_rgb_picture as in 12f, but the call WRITES through the plane pointers (the const of the
 *     type describes the ingest).  matrix and full_range of outs[i] choose the row of the table below.  HMR_GPU_RGB_PACKED8 with 3 or 4 bytes a pixel and any offset[]
 *     (the fourth byte is written as 255), _PLANAR8, _PLANAR_F32: x = (float)v / 255.0f, ONE correctly rounded binary32 division (np.float32(v) / np.float32(255)),
 *     _PLANAR_F16: that binary32 value rounded to binary16, to nearest even.  For both float forms 12f's quantisation of x gives v back for all 256 values: an output
 *     fed back through 12f is the same 8-bit picture.  Only the bytes of the rows are written - [plane + y * pitch, plane + y * pitch + row bytes).
 *     refs with dev_ssd (both NULL or both given; dev_ssd: device memory, n x 3 values): refs[i] is the caller's original RGB picture in any form of 12f (its matrix and
 *     range fields are checked but not used - except when outs is NULL: then THEY choose the row of the table); dev_ssd[3 * i + c] = the sum over width x height of
 *     (q(ref) - v)^2 for c = R, G, B, exact, q being 12f's 8-bit quantisation of the reference's sample and v the 8-bit value of the arithmetic below (also when the
 *     output form is float).  The values are overwritten, not accumulated.  hmr_gpu_psnr_rgb turns three sums into 10 * log10(255 * 255 * width * height / sum) for R,
 *     G and B, and psnr[3]: the same expression over all 3 * width * height samples; 99.99 where the sum is 0, as hmr_gpu_psnr.  Pure host code.
 *     The arithmetic is defined in integers, so that a caller can reproduce every sample (homerhevc_amd/csrc/yuv_rgb.h holds it once, for the kernel and the host):
 *       inputs: 8-bit Y [H, W] and U, V [H / 2, W / 2]; chroma sample (cx, cy) sited at the centre of the luma block (2 cx .. 2 cx + 1, 2 cy .. 2 cy + 1) - what 12f makes.
 *       chroma at luma position (x, y): bilinear, scaled by 16, not rounded.  Rows, with cy = y >> 1: an even y takes rows cy - 1 (weight 1) and cy (weight 3), an odd y
 *         rows cy (weight 3) and cy + 1 (weight 1); columns: the same rule with x; indices are clamped to the plane, so an edge sample gets the full weight.
 *         C16 = sum of wy wx C, 0 .. 4080; a flat plane gives exactly 16 C.
 *       per pixel:  L = 16 Ky (Y - yoff), U' = U16 - 2048, V' = V16 - 2048
 *                   R = clamp((L + Rv V' + 131072) >> 18, 0, 255)
 *                   G = clamp((L + Gu U' + Gv V' + 131072) >> 18, 0, 255)
 *                   B = clamp((L + Bu U' + 131072) >> 18, 0, 255);  >> is an arithmetic shift of a 32-bit signed value
 *       matrix, range     Ky      Rv      Gu      Gv       Bu      yoff
 *       BT.601 limited    19077   26149   -6419   -13320   33050   16
 *       BT.601 full       16384   22970   -5638   -11700   29032   0
 *       BT.709 limited    19077   29372   -3494   -8731    34610   16
 *       BT.709 full       16384   25802   -3069   -7670    30402   0
 *     Each coefficient is round(real x 2^14) of the inverse BT matrix (255 / 219 and 255 / 224 x 2 (1 - Kr), ... in limited range; 1 and 2 (1 - Kr), ... in full range).
 *     Every output is within 0.52 of the real-valued formula applied to the same bilinear chroma; flat chroma 128 gives R = G = B, in full range R = G = B = Y at all 256
 *     levels; a flat picture of any colour through 12f and back returns each channel within 1 (full range) or 2 (limited range).
 *     consumer_stream: as in 12e, word for word.  The launch runs on the first encoder's stream behind an event recorded on consumer_stream and behind whatever the
 *     encoders' streams and the streams that wrote the final pictures hold; consumer_stream and the encoders' streams go on behind the launch; the host waits for
 *     nothing.  The producer of the reference pictures must be on consumer_stream, or ordered before it.
 *     Refused with HMR_GPU_ERR_ARG and a text (hmr_gpu_last_error) before anything is queued, every encoder left working: n outside 1 .. 512, NULL encs or which, a NULL
 *     encoder, encoders on different devices, both outs and refs NULL, refs without dev_ssd or the reverse, which below -1 or a slot that does not exist, which = -1 on
 *     an encoder without an encoded picture, whatever hmr_gpu_rgb_picture_check refuses for outs[i] or refs[i] at the encoder's picture size, sums for a picture wider
 *     than 8192 samples, an output plane, a reference plane or dev_ssd that hipPointerGetAttributes does not report as device memory of the encoders' device.
 *     hmr_gpu_rgb_from_yuv_host: the same arithmetic in a plain loop over HOST memory, from tightly packed I420 planes (y: width x height; u, v: width / 2 x height / 2)
 *     into a descriptor whose planes are host pointers.  hmr_gpu_rgb_ssd_host: the same sums between two RGB pictures in host memory, in any two forms.  Both are pure
 *     host code - no device, no context - and refuse what hmr_gpu_rgb_picture_check refuses and NULL arguments.  hmr_gpu_psnr_rgb refuses NULL arguments and an odd or
 *     non-positive width or height.
 *     Out of scope: other chroma sitings or upsampling filters, 10-bit or bfloat16 output (12k brings deeper pictures IN; what comes out stays 8-bit), a colour description in the VUI (12f: the stream does not say which matrix
 *     or range was used), SSIM in the RGB domain, scaled RGB export.
 * ------------------------------------------------------------------------------------------------ */
int hmr_gpu_enc_export_pictures_rgb_device(hmr_gpu_enc **encs, int n, const int *which, const hmr_gpu_rgb_picture *outs, const hmr_gpu_rgb_picture *refs, uint64_t *dev_ssd,
					   void *consumer_stream);
int hmr_gpu_enc_export_picture_rgb_device(hmr_gpu_enc *enc, int which, const hmr_gpu_rgb_picture *out, const hmr_gpu_rgb_picture *ref, uint64_t *dev_ssd, void *consumer_stream);
int hmr_gpu_rgb_from_yuv_host(const uint8_t *y, const uint8_t *u, const uint8_t *v, int width, int height, const hmr_gpu_rgb_picture *out);
int hmr_gpu_rgb_ssd_host(const hmr_gpu_rgb_picture *a, const hmr_gpu_rgb_picture *b, int width, int height, uint64_t ssd[3]);
int hmr_gpu_psnr_rgb(const uint64_t ssd[3], int width, int height, double psnr[4]);

/* ------------------------------------------------------------------------------------------------
 * 12j. A resolution ladder from RGB pictures in device memory: colour conversion and downscaling inside the ingest (no counterpart in the reference)
 *     A renderer or a tensor library holds a float [3, H, W] or packed RGBA frame that is wanted at several smaller sizes - or at one smaller size only, or as a crop.
 *     hmr_gpu_enc_load_sources_scaled_rgb_device fills picture slots of n encoders (1 .. 512) from RGB pictures that are LARGER than (or as large as) the encoders'
 *     pictures with ONE launch of a kernel (k_rgb_ladder, picture_io.hip).  No new formula: the slot is the composition of two sections above, bit for bit,
 *       out = 12g's area average (source size -> encoder size, every plane on its own, one rounding) of the 8-bit 4:2:0 picture that 12f's conversion makes of the RGB
 *             source at the source's size
 *     so that for every entry  slot == hmr_gpu_scale_host(hmr_gpu_rgb_convert_host(rgb)) : what loading a source-sized encoder with 12f, exporting its slot and loading
 *     that picture with 12g gives, and a ladder whose top rung is encoded from the RGB picture itself (12f) stays consistent with its lower rungs.  The 8-bit picture
 *     in between never exists in memory: 12f's luma is a function of one pixel and its chroma of one 2 x 2 block, so the kernel converts each source sample in
 *     registers and accumulates 12g's weighted sums directly.  Luma and chroma are produced by different workgroups, each of which reads the RGB source: it is read
 *     twice per entry.
 *     Every output is within 1.01 of the real-valued area average of the real-valued BT formula: 0.51 from 12f for every converted sample, which an average with
 *     weights that sum to 1 cannot enlarge, plus 0.5 from 12g's single rounding.
 *     Formats, channel orders, matrices, ranges, sizes and ratios may be mixed within a call, and the same source may appear in any number of entries.  An entry whose
 *     source has the encoder's size is legal and gives exactly what hmr_gpu_enc_load_sources_rgb_device gives.  The source is any of 12f's forms at any base address
 *     and pitch (float planes aligned to their element), so a crop is just a view.
 *     It carries the contract of 12d word for word: the launch runs on the first encoder's stream behind what producer_stream holds now, producer_stream and the
 *     other encoders' streams go on behind it, the host waits for nothing (but for a slot that has to be allocated first); only the bytes of the source's rows are
 *     read, nothing outside width x height of the slot is written; a slot filled this way is indistinguishable, to every encode call, from one filled by
 *     hmr_gpu_enc_load_sources_device with the host-made I420 picture.  hmr_gpu_enc_export_sources_device (12f) returns what the slot holds.
 *     Refused with HMR_GPU_ERR_ARG and a text (hmr_gpu_last_error) before anything is queued, every encoder left working: what 12d refuses; what
 *     hmr_gpu_rgb_picture_check refuses for the SOURCE's size (hmr_gpu_scaled_rgb_picture.width, .height); what hmr_gpu_scale_check refuses for (source size ->
 *     encoder size); a plane that hipPointerGetAttributes does not report as device memory of the encoders' device.
 *     hmr_gpu_scale_rgb_host: the same arithmetic in a plain loop over HOST memory - the descriptor's planes are host pointers here - into tightly packed I420 planes
 *     (y: dst_w x dst_h; u, v: dst_w / 2 x dst_h / 2): every output sums its taps and converts the pixel or the 2 x 2 block under each tap, no picture in between.  No
 *     device, no context.  It refuses what hmr_gpu_rgb_picture_check and hmr_gpu_scale_check refuse and NULL arguments, except that it takes any ratio, as
 *     hmr_gpu_scale_host does.  A utility; it is not a fallback for encoding.
 *     Out of scope: averaging in RGB before converting (a different, new arithmetic), upscaling, one read of a source shared by several entries, other chroma sitings.
 * ------------------------------------------------------------------------------------------------ */
typedef struct hmr_gpu_scaled_rgb_picture {
	hmr_gpu_rgb_picture pic;       /* the SOURCE picture, as in 12f */
	int32_t width, height;         /* the SOURCE's size */
} hmr_gpu_scaled_rgb_picture;      /* 88 bytes */
int hmr_gpu_enc_load_sources_scaled_rgb_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_scaled_rgb_picture *pics, void *producer_stream);
int hmr_gpu_enc_load_source_scaled_rgb_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_scaled_rgb_picture *pic, void *producer_stream);
int hmr_gpu_scale_rgb_host(const hmr_gpu_scaled_rgb_picture *pic, int dst_w, int dst_h, uint8_t *y, uint8_t *u, uint8_t *v);

/* ------------------------------------------------------------------------------------------------
 * 12k. Y'CbCr pictures of more than 8 bits, 4:2:2 and 4:4:4 in device memory: rounding to 8-bit 4:2:0 inside the ingest (no counterpart in the reference)
 *     12d takes 8-bit 4:2:0 as I420 or NV12.  A decoder leaves more than that on the GPU: P010 / P016 (16-bit containers, the sample in the high bits) and
 *     yuv420p10le-style planes (the sample in the low bits) from every 10-bit source; planar or semi-planar 4:2:2 and 4:4:4 from JPEG and mezzanine decoders; packed
 *     YUYV / UYVY (and Y210 / Y216) from capture.  hmr_gpu_enc_load_sources_yuv_device brings n such pictures (1 .. 512; forms may be mixed within a call) to 8-bit
 *     4:2:0 and into picture slots of their encoders with ONE launch of a bandwidth-bound kernel (k_ingest_yuv, picture_io.hip): every source sample is read once,
 *     nothing is written but the slot.  What the encoder encodes does not change: it stays 8-bit 4:2:0.
 *     The arithmetic is defined in integers, so that a caller can reproduce every sample (homerhevc_amd/csrc/yuv_depth.h holds it once, for the kernel and the host).
 *     A source sample is an unsigned integer in a container of 1 byte (bits == 8) or 2 bytes (bits 9 .. 16, little endian).
 *       raw    = the container's value
 *       v      = msb_aligned ? raw >> (16 - bits) : min(raw, 2^bits - 1)
 *       s      = bits - 8
 *       luma:    Y(x, y) = min(255, (v + r(s)) >> s)                          r(t) = t ? 1 << (t - 1) : 0
 *       chroma:  n = 2^k taps, S = their sum of v
 *                C(cx, cy) = min(255, (S + r(s + k)) >> (s + k))
 *         4:2:0  k = 0: the sample (cx, cy)
 *         4:2:2  k = 1: column cx of chroma rows 2 cy and 2 cy + 1           (vertical average; horizontal siting untouched)
 *         4:4:4  k = 2: the 2 x 2 block (2 cx .., 2 cy ..)                    (the block's average, sited at its centre: what 12f makes)
 *     ONE rounding and nothing in between, in unsigned 32-bit arithmetic: 4 x 65535 + 2^9 < 2^32.  So:
 *       - every output is within 0.5 of the real-valued average of v / 2^s; where that average is >= 255.5 the result is 255 (10-bit 1023 -> 255, four 16-bit
 *         65535 -> 255);
 *       - 8-bit 4:2:0 is the identity: the slot is bit for bit what hmr_gpu_enc_load_sources_device gives for the same planes;
 *       - an 8-bit picture widened to any depth (v << s, in either alignment) comes back unchanged, for every chroma format when the widened chroma is constant over
 *         its taps;
 *       - 10-bit limited range stays limited range: 64 -> 16, 940 -> 235, 960 -> 240.
 *     There is NO range conversion, no tone mapping, no dithering and no change of the transfer function: a PQ or HLG source stays PQ or HLG in 8 bits.  The stream
 *     carries no colour description (12f): whoever decodes it has to be told by other means.
 *     Layouts.  sb: the container's bytes; chroma width Wc = W / 2 for 4:2:0 and 4:2:2, W for 4:4:4; chroma rows Hc = H / 2 for 4:2:0, H otherwise.
 *       PLANAR       planes Y, U, V; pitches at least W sb, Wc sb, Wc sb; offset[] all 0.
 *       SEMIPLANAR   planes Y and one plane of interleaved pairs, plane[2] NULL; pitches at least W sb, 2 Wc sb; offset[0] = 0, offset[1] and offset[2] in {0, 1},
 *                    distinct: which sample of a pair is U and which is V (NV12 / P010: 0, 1; NV21: 1, 0).
 *       PACKED422    plane[0] only, groups of four samples per two pixels; pitch at least 2 W sb; chroma = HMR_GPU_CHROMA_422 only.  offset[0] in {0, 1} is the
 *                    group's first luma sample, the second is at offset[0] + 2; offset[1] and offset[2] are the two remaining positions (YUYV: 0, 1, 3; UYVY: 1, 0, 2;
 *                    YVYU: 0, 3, 1; VYUY: 1, 2, 0).  Y210 / Y216 are PACKED422 with 16-bit containers.
 *     16-bit containers need planes and pitches that are multiples of 2.  Any base address and pitch otherwise, so a crop is just a view.
 *     hmr_gpu_yuv_picture_check: pure host, like hmr_gpu_picture_check; names the field.  Refused: a NULL descriptor; an unknown format or chroma; bits outside
 *     8 .. 16; msb_aligned outside 0 / 1, or 1 with bits 8 or 16 (there is nothing to align); non-zero reserved; an odd or non-positive width or height; PACKED422
 *     with another chroma; an offset outside what its format allows, or repeated; a missing plane, or a plane the format does not have; a negative pitch, or one
 *     below a row's bytes; a 16-bit plane or pitch that is not a multiple of 2.
 *     hmr_gpu_yuv_convert_host: the same arithmetic in plain loops over HOST memory - the descriptor's planes are host pointers here - into tightly packed I420 planes
 *     (y: width x height, u, v: width / 2 x height / 2).  No device, no context.  It refuses what the check refuses, before a pointer is followed, and NULL outputs.
 *     A utility in the spirit of hmr_gpu_rgb_convert_host; it is not a fallback for encoding.
 *     The load calls carry the contract of 12d word for word: the launch runs on the first encoder's stream behind what producer_stream holds now, producer_stream
 *     and the other encoders' streams go on behind it, the host waits for nothing (but for a slot that has to be allocated first); only the bytes of the rows are
 *     read - [plane + y * pitch, plane + y * pitch + row bytes) -, nothing outside width x height of the slot is written; a slot filled this way is indistinguishable,
 *     to every encode call, from one filled by hmr_gpu_enc_load_sources_device with the converted I420 picture.  hmr_gpu_enc_export_sources_device (12f) returns
 *     what the slot holds.  Refused as in 12d, plus whatever hmr_gpu_yuv_picture_check refuses for the encoder's picture size.
 *     Out of scope: upsampling chroma; other sitings or filters; dithering; range, matrix or transfer conversion; big-endian samples; the 10:10:10:2 packings (v210,
 *     Y410); float Y'CbCr; high-depth or 4:2:2 / 4:4:4 OUTPUT (12e writes 8-bit 4:2:0); scaled deep sources HERE (12g takes 8-bit 4:2:0; 12l rounds and scales them in one launch); anything that changes what the
 *     encoder itself encodes.
 * ------------------------------------------------------------------------------------------------ */
enum { HMR_GPU_YUV_PLANAR = 0, HMR_GPU_YUV_SEMIPLANAR = 1, HMR_GPU_YUV_PACKED422 = 2 };
enum { HMR_GPU_CHROMA_420 = 0, HMR_GPU_CHROMA_422 = 1, HMR_GPU_CHROMA_444 = 2 };
typedef struct hmr_gpu_yuv_picture {
	int32_t format, chroma, bits, msb_aligned;   /* HMR_GPU_YUV_*; HMR_GPU_CHROMA_*; 8 .. 16; 1: the sample is in the container's high bits (P010), 0: in its low bits */
	int32_t offset[3], reserved;                 /* see the layouts above; 0 */
	const void *plane[3];                        /* device pointers (hmr_gpu_yuv_convert_host: host pointers); planes the format does not have are NULL */
	int64_t pitch[3];                            /* bytes from row to row */
} hmr_gpu_yuv_picture;                           /* 80 bytes */
int hmr_gpu_yuv_picture_check(const hmr_gpu_yuv_picture *pic, int width, int height);
int hmr_gpu_yuv_convert_host(const hmr_gpu_yuv_picture *pic, int width, int height, uint8_t *y, uint8_t *u, uint8_t *v);
int hmr_gpu_enc_load_source_yuv_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_yuv_picture *pic, void *producer_stream);
int hmr_gpu_enc_load_sources_yuv_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_yuv_picture *pics, void *producer_stream);

/* ------------------------------------------------------------------------------------------------
 * 12l. A resolution ladder from Y'CbCr pictures of more than 8 bits, 4:2:2 and 4:4:4 in device memory: rounding and downscaling inside the ingest (no counterpart
 *      in the reference)
 *     A hardware decoder leaves P010, a mezzanine is 10-bit 4:2:2, a capture card hands over UYVY or Y210 - and the picture is wanted at several smaller sizes, or
 *     at one smaller size only, or as a crop.  hmr_gpu_enc_load_sources_scaled_yuv fills picture slots of n encoders (1 .. 512) from Y'CbCr pictures in any of 12k's
 *     forms that are LARGER than (or as large as) the encoders' pictures with ONE launch of a kernel (k_yuv_ladder, picture_io.hip).  No new formula: the slot is the
 *     composition of two sections above, bit for bit,
 *       out = 12g's area average (source size -> encoder size, every plane on its own, one rounding) of the 8-bit 4:2:0 picture that 12k's rounding makes of the
 *             source at the source's size
 *     so that for every entry  slot == hmr_gpu_scale_host(hmr_gpu_yuv_convert_host(yuv)) : what loading a source-sized encoder with 12k, exporting its slot and loading
 *     that picture with 12g gives in three launches, and a ladder whose top rung is loaded through 12k stays consistent with its lower rungs.  The 8-bit picture in
 *     between never exists in memory: 12k's luma sample is a function of one container and its chroma sample of 1, 2 or 4 containers of one plane, so the kernel
 *     rounds each source sample in registers and accumulates 12g's weighted sums directly.  Planar and semi-planar sources are read once per entry (luma and chroma
 *     are produced by different workgroups, each of which reads its own planes); a packed source's single plane is read by both: twice per entry.
 *     With x the real-valued average of v / 2^s over a 12k sample's taps, every 12k sample is within 0.5 of min(255, x): the rounding gives at most 0.5 below 255,
 *     the clamp gives exactly 255 above it.  An average with weights that sum to 1 cannot enlarge that, and 12g's single rounding adds at most 0.5: every output is
 *     within 1.0 of the real-valued area average of the min(255, x) planes.
 *     Forms, depths, alignments, chroma formats, sizes and ratios may be mixed freely within a call, and the same source may appear in any number of entries.  An
 *     entry whose source has the encoder's size is legal and gives exactly what hmr_gpu_enc_load_sources_yuv_device gives.  The source is any of 12k's forms at any
 *     base address and pitch (16-bit containers: multiples of 2), so a crop is just a view.
 *     The two load entries take device pictures like their siblings; their names deliberately do not end in _device.
 *     It carries the contract of 12d word for word: the launch runs on the first encoder's stream behind what producer_stream holds now, producer_stream and the
 *     other encoders' streams go on behind it, the host waits for nothing (but for a slot that has to be allocated first); only the bytes of the source's rows are
 *     read, nothing outside width x height of the slot is written; a slot filled this way is indistinguishable, to every encode call, from one filled by
 *     hmr_gpu_enc_load_sources_device with the host-made I420 picture.  hmr_gpu_enc_export_sources_device (12f) returns what the slot holds.
 *     Refused with HMR_GPU_ERR_ARG and a text (hmr_gpu_last_error) before anything is queued, every encoder left working: what 12d refuses; what
 *     hmr_gpu_yuv_picture_check refuses for the SOURCE's size (hmr_gpu_scaled_yuv_picture.width, .height); what hmr_gpu_scale_check refuses for (source size ->
 *     encoder size); a plane that hipPointerGetAttributes does not report as device memory of the encoders' device.
 *     hmr_gpu_scale_yuv_host: the same arithmetic in a plain loop over HOST memory - the descriptor's planes are host pointers here - into tightly packed I420 planes
 *     (y: dst_w x dst_h; u, v: dst_w / 2 x dst_h / 2): every output sums its taps and rounds the container or the 1, 2 or 4 containers under each tap, no picture in
 *     between.  No device, no context.  It refuses what hmr_gpu_yuv_picture_check and hmr_gpu_scale_check refuse and NULL arguments, except that it takes any ratio,
 *     as hmr_gpu_scale_rgb_host does: the bound of 8 is the kernel's.  A utility; it is not a fallback for encoding.
 *     Out of scope: a single rounding from the deep samples (within 0.5 instead of 1.0, but a new arithmetic that no longer equals the three-launch path or a top
 *     rung loaded through 12k); range, matrix or transfer conversion and tone mapping; deep or 4:2:2 output; upscaling; ratios above 8 on the device.
 * ------------------------------------------------------------------------------------------------ */
typedef struct hmr_gpu_scaled_yuv_picture {
	hmr_gpu_yuv_picture pic;       /* the SOURCE picture, as in 12k */
	int32_t width, height;         /* the SOURCE's size */
} hmr_gpu_scaled_yuv_picture;      /* 88 bytes; width at 80, height at 84 */
int hmr_gpu_enc_load_sources_scaled_yuv(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_scaled_yuv_picture *pics, void *producer_stream);
int hmr_gpu_enc_load_source_scaled_yuv(hmr_gpu_enc *enc, int slot, const hmr_gpu_scaled_yuv_picture *pic, void *producer_stream);
int hmr_gpu_scale_yuv_host(const hmr_gpu_scaled_yuv_picture *pic, int dst_w, int dst_h, uint8_t *y, uint8_t *u, uint8_t *v);

/* ------------------------------------------------------------------------------------------------
 * 12m. Scene-cut statistics of a frame against its predecessor, left in device memory: batched motion-compensated cost sums
 *     Every encode call takes an image_type; nothing in the library said when to pass an intra picture.  The reference's own detector (hmr_motion_inter.c:3791) fires
 *     in the middle of a P frame, after a tenth of the partitions, adjusts costs and the GOP, and leaves the cut frame a P picture; it runs per encoder, so the rungs
 *     of a ladder decide independently.  hmr_gpu_enc_cut_stats leaves, for n encoders (1 .. 512, sizes mixed), eight exact statistics of the picture in slot
 *     slots[i] of encs[i] (cur) against the picture in slot prev_slots[i] of the same encoder (prev) with ONE call: a launch of k_cut (picture_io.hip) over the int16
 *     planes of the two slots and a small finishing kernel behind it, no host synchronisation.  It needs no encoded picture: it works before the first encode, on
 *     whatever the two slots hold when the launch runs - whatever form the frames arrived in (12d, 12f, 12g, 12j, 12k, 12l).
 *     The arithmetic is defined in integers, so that a caller can reproduce every value (homerhevc_amd/csrc/cut_stats.h holds it once, for the kernel and the host).
 *     cur and prev are 8-bit 4:2:0 samples of a W x H picture.  Every size the frame encoder accepts is a multiple of 8, so luma is an exact grid of 8 x 8 BLOCKS.
 *     The call leaves HMR_GPU_CUT_VALUES = 8 signed 64-bit values per picture, each exact in any order of addition:
 *       0, 1, 2  SAD_Y, SAD_U, SAD_V   the sum of abs(cur - prev) over the plane
 *       3        HIST                  the sum over v = 0 .. 255 of abs(hc[v] - hp[v]), hc and hp being the luma histograms of cur and prev; it lies in 0 .. 2 W H
 *       4        INTRA                 the sum of act(b) over the blocks
 *       5        INTER                 the sum of min(64 msad(b), act(b)) over the blocks
 *       6        NINTRA                the number of blocks with act(b) < 64 msad(b) (strict)
 *       7        LUMA                  the sum of cur's luma samples (for fades: the caller keeps the previous value)
 *     The per-block terms, for the luma block b at (bx, by):
 *       act(b)   the sum over the block's 64 samples x of abs(64 x - S), S the block's sample sum: the mean-removed deviation, scaled by 64 so that nothing is
 *                rounded.  At most 522 240 (32 samples of 255 and 32 of 0).
 *       msad(b)  the minimum, over the valid integer vectors, of the sum over the 64 samples of abs(cur(bx + i, by + j) - prev(bx + dx + i, by + dy + j)).
 *       valid    (dx, dy) in [-R, R]^2, R = HMR_GPU_CUT_RANGE = 8, for which the displaced block lies wholly inside the picture: 0 <= bx + dx, bx + dx + 8 <= W,
 *                and likewise in y.  (0, 0) is always valid, and an 8 x 8 picture has only that vector.
 *     The two entries on encoders take device memory like their siblings; their names deliberately do not end in _device, as 12l's.
 *     Only the minimum VALUE enters a sum, so no tie-break exists to get wrong.  No sample outside W x H is read: the slots' margins are never looked at.
 *     dev_stats (device memory, n x 8 values): dev_stats[8 * i + k] = value k of encs[i].  The same encoder may appear more than once.
 *     consumer_stream: as in 12h, word for word.  The launch runs on the first encoder's stream behind an event recorded on consumer_stream (the consumer may still be
 *     using dev_stats) and behind whatever the encoders' streams hold (a load into a slot); dev_stats and the library's histogram bins (2 x 256 32-bit counts per
 *     picture, owned by the first encoder) are zeroed on that stream in front of the launch.  Behind the launch the library records an event that consumer_stream and
 *     the streams of all the call's encoders wait for: what the caller queues on consumer_stream after the call sees the values, a later load into either slot runs
 *     after the kernel has read the pictures.  The host waits for nothing in either direction (but for the bins, allocated at the first call an encoder leads).
 *     Refused with HMR_GPU_ERR_ARG and a text (hmr_gpu_last_error) before anything is queued, every encoder left working: n outside 1 .. 512, NULL encs, slots,
 *     prev_slots or dev_stats, a NULL encoder, encoders on different devices, a slot or a previous slot that does not exist, slots[i] == prev_slots[i], dev_stats that
 *     hipPointerGetAttributes does not report as device memory of the encoders' device.
 *     hmr_gpu_cut_stats_host: the same arithmetic in plain nested loops over two 8-bit pictures in HOST memory - the descriptors' planes are host pointers here; I420
 *     or NV12 (the two may differ), any pitch - into stats[8].  No device, no context.  It refuses what hmr_gpu_picture_check refuses for either picture, a width or
 *     height that is not a positive multiple of 8, and NULL stats.
 *     hmr_gpu_cut_score: four correctly rounded double quotients of exact integers (every operand is exact below 2^53).  Pure host code.
 *       score[0] = SAD_Y / (W H)          the mean absolute luma difference, 0 .. 255
 *       score[1] = HIST / (2 W H)         0 .. 1
 *       score[2] = NINTRA / blocks        the share of blocks that motion compensation from prev does not explain, 0 .. 1; blocks = W H / 64
 *       score[3] = INTER / INTRA          0 .. 1, or 1.0 when INTRA is 0
 *     It refuses NULL arguments, a width or height that is not a positive multiple of 8, a value outside its range (below 0; SAD_Y, LUMA above 255 W H; SAD_U, SAD_V
 *     above 255 W H / 4; HIST above 2 W H; INTRA, INTER above 522 240 blocks; NINTRA above blocks) and INTER above INTRA.
 *     Out of scope: sub-sample motion, vectors or per-block maps as outputs, ranges other than 8, chroma in the search, lookahead over more than one frame, fade
 *     handling beyond exposing LUMA.  The reference's own detector is unchanged.
 * ------------------------------------------------------------------------------------------------ */
#define HMR_GPU_CUT_VALUES 8
#define HMR_GPU_CUT_RANGE 8
int hmr_gpu_enc_cut_stats(hmr_gpu_enc **encs, int n, const int *slots, const int *prev_slots, int64_t *dev_stats, void *consumer_stream);
int hmr_gpu_enc_cut_stats_one(hmr_gpu_enc *enc, int slot, int prev_slot, int64_t *dev_stats, void *consumer_stream);
int hmr_gpu_cut_stats_host(const hmr_gpu_picture *cur, const hmr_gpu_picture *prev, int width, int height, int64_t stats[8]);
int hmr_gpu_cut_score(const int64_t stats[8], int width, int height, double score[4]);

/* ------------------------------------------------------------------------------------------------
 * 13. Phase planes of a reference picture
 *     Replaces the per-block interpolation calls of the motion search and of motion compensation - the sixteen planes of
 *     hmr_half_pixel_estimation_luma_hm / hmr_quarter_pixel_estimation_luma_hm (hmr_motion_inter.c:395,442) and
 *     hmr_motion_compensation_luma / _chroma (:1779,1860), all through low_level_funcs_t.interpolate_luma / interpolate_chroma
 *     (hmr_private.h:1077-1078, stage rules hmr_motion_inter.c:240-391) - by ONE bandwidth-bound pass per reference picture.
 *     All pointers are device memory.  pic_y / pic_u / pic_v: the padded int16 planes from the first element of their allocation,
 *     stride x rows elements each (strides multiples of 4).  out_y: 16 x stride_y x rows_y bytes, plane fy * 4 + fx = the picture
 *     displaced by (fx, fy) quarter samples, clipped to 8 bits like the final stage of the interpolation; out_u / out_v: 64 planes
 *     each, plane fy * 8 + fx in eighth samples (pic_u / pic_v / out_u / out_v may be NULL: luma only).  The planes are
 *     row-interleaved - row y of plane f starts at byte (y * 16 + f) * stride_y (chroma: (y * 64 + f) * stride_c) - so that the
 *     window a CTU reads of all of them is one stretch of memory.  Taps run over row ends
 *     linearly, as the reference's pointer arithmetic does; taps outside the allocation read zero.
 * ------------------------------------------------------------------------------------------------ */
int hmr_gpu_subpel_planes(hmr_gpu_ctx *ctx, const int16_t *pic_y, const int16_t *pic_u, const int16_t *pic_v, int stride_y, int rows_y, int stride_c, int rows_c,
			  uint8_t *out_y, uint8_t *out_u, uint8_t *out_v);

/* ------------------------------------------------------------------------------------------------
 * 14. Measurement aid (no counterpart in the reference): the vector-instruction issue rate of the device
 *     k_encode_pool is bound by the instruction issue of a few wavefronts per CU and by the latency of its dependent chains, not by HBM bandwidth; bench.py prices it
 *     against wave-instructions per second.  This measures that ceiling on the device at hand: every CU runs waves_per_simd (1 .. 4) wavefronts per SIMD, each a
 *     loop of 64 integer multiply-adds without memory accesses - on eight independent accumulators, or (dependent != 0) as ONE chain, the rate a single dependent
 *     instruction stream reaches.  *wave_instr_per_s: vector instructions per second of all wavefronts together; *ms (may be NULL): the launch's duration.
 * ------------------------------------------------------------------------------------------------ */
int hmr_gpu_probe_valu_issue(hmr_gpu_ctx *ctx, int waves_per_simd, int dependent, double *wave_instr_per_s, double *ms);
/* the same for one instruction kind: op 0 v_mad_u32_u24, 1 v_add_u32, 2 v_mov_b32, 3 v_perm_b32, 4 s_add_u32 (scalar unit) */
int hmr_gpu_probe_issue(hmr_gpu_ctx *ctx, int op, int waves_per_simd, int dependent, double *wave_instr_per_s, double *ms);

/* ------------------------------------------------------------------------------------------------
 * 15. Test aid: the block primitives the frame encoder's CTU walk runs (homerhevc_amd/csrc/enc/enc_prims.h), one call at a time
 *     k_encode_pool does not go through the table kernels of sections 1 - 7: its worker wavefront runs SPMD primitives of its own on data in LDS.  These entries run exactly
 *     those primitives - one wavefront, as in the walk - behind the flat signatures of the table functions they restate (hmr_private.h:1063-1092; the same argument meaning as
 *     hmr_gpu_sad ... hmr_gpu_inv_quant above), so that the parity sweep of the table kernels also holds the walk's primitives to the oracle (tests/test_gpu_prims.py).
 *     hmr_gpu_prim_bytes(1): sample operands the worker keeps as bytes (source block, prediction window) are narrowed first, i.e. the byte instantiations run - for
 *     calls whose samples are 0 .. 255; hmr_gpu_prim_sad then is the motion search's multi-candidate byte SAD.  Host pointers, synchronous, default context.
 * ------------------------------------------------------------------------------------------------ */
void hmr_gpu_prim_bytes(int on);
uint32_t hmr_gpu_prim_sad(int16_t *src, uint32_t src_stride, int16_t *pred, uint32_t pred_stride, int size);
uint32_t hmr_gpu_prim_ssd16b(int16_t *src, uint32_t src_stride, int16_t *pred, uint32_t pred_stride, int size);
void hmr_gpu_prim_predict(int16_t *orig, int orig_stride, int16_t *pred, int pred_stride, int16_t *residual, int residual_stride, int size);
void hmr_gpu_prim_reconst(int16_t *pred, int pred_stride, int16_t *residual, int residual_stride, int16_t *decoded, int decoded_stride, int size);
uint32_t hmr_gpu_prim_modified_variance(int16_t *p, int size, int stride, int modif);
void hmr_gpu_prim_intra_planar(int16_t *prediction, int pred_stride, int16_t *adi_pred_buff, int adi_size, int cu_size);
void hmr_gpu_prim_intra_angular(int16_t *prediction, int pred_stride, int16_t *adi_pred_buff, int adi_size, int cu_size, int cu_mode, int is_luma);
void hmr_gpu_prim_fill_reference_samples(int16_t *decoded_corner, int stride, int n, int left, int top, int bottom_left, int top_right, int bl_size, int tr_size, int16_t *adi);
void hmr_gpu_prim_adi_filter(int16_t *adi, int16_t *out, int adi_size, int n, int strong_enabled);
void hmr_gpu_prim_transform(int16_t *block, int16_t *coeff, int block_stride, int n, int is_dst);
void hmr_gpu_prim_itransform(int16_t *block, int16_t *coeff, int block_stride, int n, int is_dst);
void hmr_gpu_prim_quant(int16_t *src, int16_t *dst, int16_t *delta_u, int scan_mode, int depth, int comp, int is_intra, int slice_is_intra, int sign_hiding, int *ac_sum,
			int cu_size, int per, int rem);
void hmr_gpu_prim_inv_quant(int16_t *src, int16_t *dst, int depth, int comp, int is_intra, int cu_size, int per, int rem);
/* The motion search's multi-candidate byte SAD (multi_sad_u8<MAXC>, the instantiations the walk uses: maxc = 4, 8, 9), every result.  src: the source block, n rows at a pitch
 * of 64 bytes (64 x n bytes are read); plane: plane_bytes bytes; cand_off: ncalls lists of maxc byte offsets into the plane, -1 = a candidate that is skipped (a NULL pointer
 * in the walk: its result is 0); stride: the plane's row pitch; n: 8, 16, 32 or 64; out: ncalls x maxc sums.  One launch, a workgroup per list.  HMR_GPU_ERR_ARG (nothing is
 * launched) for another maxc or n, a stride below 1, or a candidate block that does not lie inside the plane. */
int hmr_gpu_prim_multi_sad(int maxc, const uint8_t *src, const uint8_t *plane, size_t plane_bytes, const int64_t *cand_off, int ncalls, int stride, int n, uint32_t *out);
/* The motion search of the walk (motion_estimation<WaveGrp>, homerhevc_amd/csrc/enc/enc_inter.h) - on the device a round's positions, window tests and vector costs are
 * computed in the lanes, a form the one-lane checker build does not have - once per case, a workgroup per case, one launch.  Every case searches for a block of
 * size x size samples (8, 16, 32 or 64) of a picture of width x height samples:
 *   src     ncases source blocks, size x size bytes each at a pitch of `size`;
 *   planes  plane_bytes bytes that hold the reference picture's sixteen luma phase planes in the addressing of section 13 (row y of plane f starts at
 *           (y * 16 + f) * stride bytes); origin: the byte offset of sample (0, 0) of plane 0.  The search reads up to one sample beyond the picture on every side
 *           (the sub-sample rounds at a picture edge): origin - 16 * stride - 1 >= 0 and origin + (height * 16 + 15) * stride + width + 1 <= plane_bytes;
 *   a case  the block's position (gx, gy: 0 .. width - size, 0 .. height - size), the AMVP list (0 .. 2 vectors in quarter samples) the vector cost is taken against,
 *           the search list (0 .. 3 predictor vectors in quarter samples), corr (the vector cost is corr x the distance to the nearest AMVP vector, >= 0), action (bit 0
 *           the integer search, bit 1 the half-sample round, bit 2 the quarter-sample round - which only runs behind the half-sample round) and, for an action without
 *           the integer search, the vector the sub-sample rounds start from (quarter samples; its whole-sample part must lie inside the search window);
 *   out     per case the vector (quarter samples), its sub-sample part and the SAD the search returns.
 * All vector components -32768 .. 32767.  HMR_GPU_ERR_ARG (nothing is launched) for anything outside these ranges. */
typedef struct hmr_gpu_prim_me_case {
	int32_t gx, gy;
	int32_t n_amvp, amvp[2][2];
	int32_t n_search, search[3][2];
	int32_t action;
	int32_t start[2];
	int32_t reserved;        /* 0 */
	double corr;
} hmr_gpu_prim_me_case;      /* 80 bytes */
typedef struct hmr_gpu_prim_me_out {
	int32_t mv[2], subpix[2];
	uint32_t sad;
} hmr_gpu_prim_me_out;       /* 20 bytes */
int hmr_gpu_prim_motion_search(const hmr_gpu_prim_me_case *cases, int ncases, int size, const uint8_t *src, const uint8_t *planes, size_t plane_bytes, int64_t origin, int stride,
			       int width, int height, hmr_gpu_prim_me_out *out);

/* ------------------------------------------------------------------------------------------------
 * 16. Test aid: the device-only forms of the CTU walk, one step at a time on a synthetic worker
 *     The merge tiles (homerhevc_amd/csrc/enc/enc_quad.h quad_chain: the inter TU chains of all merge slots of an 8 x 8 or 16 x 16 CU in one matrix-core tile) and the
 *     two-halves instantiation of the inter TU chain (encode_inter_tu<PairGrp>: the helper wavefront's U and V plane side by side) exist on the device only.  This entry
 *     lays one worker's LDS out as k_encode_pool does, fills what a step reads from the case, runs the step as the walk calls it and returns what it left
 *     (tests/test_gpu_walk_forms.py).  Host pointers, synchronous, default context: one upload, one launch, one download per call.
 *     arena: every byte the cases read, addressed by byte offsets:
 *       curr, pred   6144 bytes each: the worker's source / prediction windows of the CTU - 64 x 64 luma at pitch 64, then U and V, 32 x 32 at pitch 32 (multiples of 4;
 *                    pred may be -1 for a QUAD step, which does not read it);
 *       sub_y, sub_c FrameCtx::sub_y / sub_c[2]: the first valid sample of plane 0 of the phase planes in the addressing of section 13 (row y of luma plane f starts at
 *                    (y * 16 + f) * stride_y, chroma (y * 64 + f) * stride_c); a QUAD step reads, for slot s, the N x N bytes at
 *                    luma:   sub_y + ((mv.y & 3) * 4 + (mv.x & 3)) * stride_y + (ctu_y + y + (mv.y >> 2)) * 16 * stride_y + ctu_x + x + (mv.x >> 2),
 *                    chroma: sub_c[p] + ((mv.y & 7) * 8 + (mv.x & 7)) * stride_c + ((ctu_y >> 1) + yc + (mv.y >> 3)) * 64 * stride_c + (ctu_x >> 1) + xc + (mv.x >> 3)
 *                    with (x, y) / (xc, yc) the node's place in the CTU and mv = mv[s] (all four slots are read).
 *     node: the partition node (breadth first: 5 .. 20 the 16 x 16 CUs, 21 .. 84 the 8 x 8 CUs, both in z-order).  Steps:
 *       QUAD8_Y / QUAD8_C      quad_chain<8, luma> / quad_chroma_job(8) on an 8 x 8 CU: four slots;
 *       QUAD16_Y / QUAD16_C    quad_chain<16, luma> for slot one_slot / quad_chroma_job(16) on a 16 x 16 CU: two slots;
 *       TU                     encode_inter_tu<WaveGrp> for component comp: the node as one TU at its own depth, the prediction from the prediction window;
 *       TU_PAIR                encode_inter_tu<PairGrp>, U and V as helper_serve calls it.
 *     The two TU steps run the templates under group types of the harness's own, derived from WaveGrp and PairGrp (as WaveGrpLat is): every choice in the chain is by
 *     G::n, so the statements are the walk's, but the machine code is a second instantiation of them, not the one inside k_encode_pool (whose registers, scratch and
 *     inlining a further caller of its instantiations would change).  The QUAD steps run the walk's own instantiations.
 *     out[i]: per slot (a TU step: slot 0) and component distortion, level sum, no-residual distortion and cbf; pred / rec / lv: the slot's prediction, reconstruction and
 *     final levels, row by row - a luma step's N x N block, a chroma step's U block followed by its V block (a TU step on V alone: at the V block's place); stray (TU steps):
 *     32-bit words of the worker's windows in HBM (WorkSlow) outside the TU's level and reconstruction areas that the step changed.  Fields a step does not write are 0.
 *     Refused with HMR_GPU_ERR_ARG and a text (hmr_gpu_last_error) before anything is launched: a field outside its range, a node of the wrong size, a window or a
 *     prediction block that does not lie inside the arena.
 * ------------------------------------------------------------------------------------------------ */
enum hmr_gpu_walk_step { HMR_GPU_WALK_QUAD8_Y = 1, HMR_GPU_WALK_QUAD8_C, HMR_GPU_WALK_QUAD16_Y, HMR_GPU_WALK_QUAD16_C, HMR_GPU_WALK_TU, HMR_GPU_WALK_TU_PAIR };
typedef struct hmr_gpu_walk_case {
	int32_t step, node, comp, one_slot;
	int32_t qp, ctu_x, ctu_y, slice_type;            /* the node's QP; CtuPublic::x / y; 1 = P, 2 = I */
	int32_t sign_hiding, chroma_qp_offset, stride_y, stride_c;
	int32_t mv[4][2];                                /* QuadScratch::mv: x, y in quarter samples */
	double avg_dist, chroma_weight;
	int64_t sub_y, sub_c[2], curr, pred;
} hmr_gpu_walk_case;
typedef struct hmr_gpu_walk_out {
	uint32_t dist[4][3];
	int32_t sum[4][3];
	uint32_t raw[4][3], cbf[4][3];
	uint32_t stray, reserved[15];
	uint8_t pred[4][256];
	int16_t rec[4][256], lv[4][256];
} hmr_gpu_walk_out;
int hmr_gpu_walk_forms(const hmr_gpu_walk_case *cases, int ncases, const uint8_t *arena, size_t arena_bytes, hmr_gpu_walk_out *out);

/* ------------------------------------------------------------------------------------------------
 * 17. Test aid: the post-decision stage of one picture from given CTU records
 *     Deblocking, SAO statistics / candidates / decision, the SAO and CTU syntax through the lane-spread CABAC, the offset pass, border padding, the task scheduler
 *     and (with_planes) the phase-plane task S (homerhevc_amd/csrc/enc/enc_post.h, enc_entropy.h, enc_sao.h, subpel_task.h) run on whatever the CTU decisions of an
 *     encode happen to leave.  This entry feeds them chosen input instead (tests/test_gpu_post_tasks.py): `records` are nctu CTU records in the layout of
 *     hmr_gpu_enc_frame_ctus (hmr_gpu_enc_record_bytes() each), of which the side-info, the levels and the reconstruction (cropped to the picture) are uploaded as the
 *     CTU decisions would have left them; src_y / src_u / src_v is the 8-bit source picture (width x height, width / 2 x height / 2, tightly packed).  The frame is set up
 *     as an encode call sets it up for slice_type (1 = P, 2 = I) and slice QP qp, and the PRODUCT's own k_post_frame is launched with `groups` workgroups (1 .. 32) on
 *     `enc` (from hmr_gpu_enc_create or hmr_gpu_enc_create_serial_pool; the encoder's frame counters do not move).  No kernel, and no instantiation of a post task, exists for this entry alone.
 *     Before the launch every byte of the deblocked picture, the final picture, the five unit arrays, the sub-stream buffer and the phase planes is set to
 *     HMR_GPU_POST_POISON.  Outputs (host memory, all of them required; planes[] only with with_planes): the caller fills the sizes with hmr_gpu_enc_post_sizes, allocates,
 *     and sets the pointers; a call whose sizes are not the encoder's is refused.
 *       dbk, fin      the deblocked and the final picture: the whole padded allocations (stride x (rows + 2 margins) int16 each; sample (0, 0) at margin * stride + margin);
 *       mvx .. flags  the raster unit arrays (units entries each, units_stride per row);
 *       sao_recon, sao_coded   [nctu][3][35] int32: mode_idc, type_idc, type_aux, offset[32] of every CTU and component;
 *       bs, bytecnt   the sub-streams: row r's bytes at bs + r * row_cap, bytecnt[r] of them (without WPP: one sub-stream at bs, bytecnt[0]);
 *       cumbits       [nctu]; ctx, saved: [rows][ctx_bytes] RowEnt::ctx and RowEnt::saved of every row; errors: [4] PostPic::errors;
 *       planes        the three phase-plane allocations in the layout of section 13 (phase_bytes[] bytes).
 *     HMR_GPU_ERR_ARG with a text: a NULL pointer, groups outside 1 .. 32, slice_type, qp outside 0 .. 51, record_bytes != nctu x hmr_gpu_enc_record_bytes(), sizes that
 *     are not the encoder's.  HMR_GPU_ERR_HIP with a text, the outputs filled in as far as the launch got: a sub-stream that ran out of room (errors[0]) or the
 *     kernel's 30 s watchdog (errors[2]).
 * ------------------------------------------------------------------------------------------------ */
#define HMR_GPU_POST_POISON 0x5a
typedef struct hmr_gpu_post_out {
	int64_t plane_elems[3];                          /* sizes: hmr_gpu_enc_post_sizes */
	int64_t units, phase_bytes[3];
	int32_t nctu, rows, row_cap, ctx_bytes;
	int32_t stride_y, stride_c, margin_y, margin_c, units_stride, reserved;
	int16_t *dbk[3], *fin[3];                        /* outputs */
	int16_t *mvx, *mvy;
	int8_t *ref;
	uint8_t *uqp, *flags;
	int32_t *sao_recon, *sao_coded;
	uint8_t *bs;
	int32_t *bytecnt;
	uint32_t *cumbits;
	uint8_t *ctx, *saved;
	int32_t *errors;
	uint8_t *planes[3];
} hmr_gpu_post_out;
int hmr_gpu_enc_post_sizes(hmr_gpu_enc *enc, hmr_gpu_post_out *out);
int hmr_gpu_enc_post_records(hmr_gpu_enc *enc, int slice_type, int qp, const uint8_t *records, size_t record_bytes, const uint8_t *src_y, const uint8_t *src_u,
			     const uint8_t *src_v, int groups, int with_planes, hmr_gpu_post_out *out);

/* ------------------------------------------------------------------------------------------------
 * 18. Test aid: the worker / helper-wavefront protocol and what runs behind it, one step at a time with real helper wavefronts
 *     Every `if (HENC_HELPERS(e))` branch of the walk, helper_serve / helper_loop / helper_bg_search (k_encode.hip) and the background intra search
 *     (bg_post / bg_take / bg_quiesce) exist on the device only.  This entry launches workgroups of a worker wavefront and its helper wavefront, as k_encode_pool does
 *     (the same threads per workgroup, the same LDS size and places, entered through rows_enter); the worker builds its context as encode_row does, and for every case
 *     of its share fills what the step reads, posts HJOB_NEW_CTU, runs the step - the walk's own statements, jobs posted to and waited for on the real mailbox - and
 *     copies out what the step left; then it releases the helper (tests/test_gpu_helper_forms.py).  Host pointers, synchronous, default context: one upload, one
 *     download, and one launch for the cases of the plain helper loop plus one (the latency kernel's loop: rows_enter<true>) for the INTRA_SEARCH_BG cases.
 *     The worker's walk runs under group types of the harness's own derived from WaveGrp / WaveGrpLat, and so does the plain helper loop (section 16 says why); the
 *     latency loop, helper_serve_out and helper_bg_search are the product's own out-of-line functions.
 *     arena: every byte the cases read, addressed by byte offsets (multiples of 4; -1: none, where a step does not read it):
 *       curr, pred   6144 bytes each: the worker's source / prediction windows as in section 16;
 *       nbr          int16: the decoded samples around the block - the 2 N of the column left of it top to bottom, the corner, the 2 N of the row above it left to
 *                    right (4 N + 1) - written into the decoded window the step reads (luma: window depth + 1; chroma: the auxiliary window) before the step.  A luma
 *                    step: one array for the node's N x N block; a chroma step: one for U, then one for V, of the chroma block's size;
 *       sync         int16, a SYNC_UV step or SYNC job: the levels of U, the levels of V, the reconstruction of U, of V (Nc x Nc each, row by row) put into the source windows.
 *     node: the partition node (breadth first, children in z-order); ctu_x / ctu_y / width / height: CtuPublic::x / y and the picture size (bl_size / tr_size clip by
 *     them); nb: the node's left_nb, top_nb, left_bottom_nb, top_right_nb.  Steps:
 *       INTRA_SEARCH     intra_mode_search(g, e, node, depth of the node) as encode_intra_luma calls it, rounds of two candidates with HJOB_INTRA_SAD on the helper.
 *                        strong_intra, rd_mode (0 or 2 = RD_FAST), sqrt_lambda.  The neighbour directions: nb_dir[0] (left) / nb_dir[1] (top), 0 .. 34, go into
 *                        Work::intra_mode_buffs of the node's depth where the neighbour unit lies inside the CTU (the search reads them when seen_intra = 1:
 *                        Work::thread_seen_intra); a node on the CTU's left / top edge has no such neighbour (Enc::nb_ctus = 0: DC) and its nb_dir is -1.
 *                        out: mode, bits, cost_bits (the double best_cost as its 8 bytes), last_slog, srch_modes / srch_sads (the last round), adi, adi_f (4 N + 1).
 *       INTRA_SEARCH_BG  bg_variant TAKE: bg_post(node), the ordinary jobs[] (0 = none, SSD / INTER_TU / SYNC: HJOB_SSD, HJOB_INTER_TU (PART_2Nx2N at the node's
 *                        depth), HJOB_SYNC_CU for both chroma planes, posted and waited for one after the other as the inter evaluation does), bg_take(node): taken = 1,
 *                        mode, bits (cost_bits 0: the background search hands no cost over).  TAKE_OTHER: bg_post(bg_node), the jobs, bg_take(node) - taken = 0 -
 *                        then the worker's own search of node.  QUIESCE: bg_post(node), bg_quiesce, the worker's own search (taken = -1).  out as INTRA_SEARCH, and
 *                        job_r[k][0 .. 5]: HelperBox::r after job k (SSD: U, V; INTER_TU: distortion, level sum, no-residual distortion of U, then of V); a SYNC job
 *                        copies window 0 to window NWND - 1, whose blocks are returned in lv / rec.
 *       CHROMA_SEARCH    the candidate search of encode_intra_chroma: HJOB_CHROMA_SEARCH (U, candidates cand[0 .. 4] packed as there) on the helper,
 *                        chroma_search_comp for V on the worker.  out: sad_u, sad_v.
 *       CHROMA_TU        HJOB_CHROMA_TU for U on the helper (its own scratch), chroma_tu_comp for V on the worker, direction cu_mode, the scan by find_scan_mode,
 *                        cbf_shift[0 .. 1] the two cbf bit positions, QP from qp and chroma_qp_offset.  out per plane: pred, lv, rec, tu_dist, tu_sum, cbf_chroma.
 *       SSD_UV           HJOB_SSD for both planes as the skip evaluation posts it, the worker's luma SSD meanwhile.  out: ssd[0 .. 2] = U, V, luma.
 *       SYNC_UV          sync_motion_buffers(node, wnd[0 .. 3] = q_src, q_dst, d_src, d_dst): HJOB_SYNC_CU for both planes, the worker's luma copy meanwhile.
 *                        out: lv / rec = the destination windows' chroma blocks.
 *     pred / lv / rec hold plane U at [0], V at [1], Nc x Nc row by row.
 *     stray (every step): before a step every int16 of the worker's windows in HBM (WorkSlow) holds 0x1234.  After it the harness puts that value back over what it
 *     wrote itself (the nbr samples, a SYNC step's source blocks) and over the blocks the step is meant to write (a TU's levels and reconstruction, a SYNC step's
 *     destination chroma blocks; the luma blocks a SYNC_UV step copies hold that value on both sides); stray is the number of 32-bit words of WorkSlow that then hold anything else.
 *     Refused with HMR_GPU_ERR_ARG and a text (hmr_gpu_last_error) before anything is launched: "step"; "step (the library was built with a helper per chroma plane)"
 *     (HENC_NHELP = 2: every step); "node"; "node (a chroma step needs a CU of 8 or more)"; "node (an INTER_TU job: a CU of 8 to 32)"; "bg_variant"; "bg_node"
 *     (TAKE_OTHER: another node of the same depth; else equal to node); "jobs"; "ctu_x / ctu_y"; "width / height" (the node's block inside the picture); "nb";
 *     "strong_intra / rd_mode / seen_intra"; "nb_dir"; "sqrt_lambda"; "qp"; "chroma_qp_offset"; "slice_type"; "sign_hiding"; "avg_dist / chroma_weight"; "cand";
 *     "cu_mode"; "cbf_shift"; "wnd"; "curr"; "pred"; "nbr"; "sync".
 * ------------------------------------------------------------------------------------------------ */
enum hmr_gpu_helper_step { HMR_GPU_HELPER_INTRA_SEARCH = 1, HMR_GPU_HELPER_INTRA_SEARCH_BG, HMR_GPU_HELPER_CHROMA_SEARCH, HMR_GPU_HELPER_CHROMA_TU, HMR_GPU_HELPER_SSD_UV,
			   HMR_GPU_HELPER_SYNC_UV };
enum hmr_gpu_helper_bg { HMR_GPU_HELPER_BG_TAKE = 0, HMR_GPU_HELPER_BG_TAKE_OTHER, HMR_GPU_HELPER_BG_QUIESCE };
enum hmr_gpu_helper_job { HMR_GPU_HELPER_JOB_NONE = 0, HMR_GPU_HELPER_JOB_SSD, HMR_GPU_HELPER_JOB_INTER_TU, HMR_GPU_HELPER_JOB_SYNC };
typedef struct hmr_gpu_helper_case {
	int32_t step, node, bg_node, bg_variant;
	int32_t ctu_x, ctu_y, width, height;
	int32_t strong_intra, rd_mode, seen_intra, slice_type;
	int32_t nb[4];
	int32_t nb_dir[2], qp, chroma_qp_offset;
	int32_t sign_hiding, cu_mode, cbf_shift[2];
	int32_t cand[5], jobs[4], wnd[4], reserved[3];
	double sqrt_lambda, chroma_weight, avg_dist;
	int64_t curr, pred, nbr, sync;
} hmr_gpu_helper_case;
typedef struct hmr_gpu_helper_out {
	int32_t mode, bits, taken, last_slog;
	uint64_t cost_bits;
	int64_t srch_sads[5];
	int32_t srch_modes[6];
	uint32_t sad_u[5], sad_v[5];
	uint32_t job_r[4][6];
	int32_t tu_dist[2], tu_sum[2];
	uint32_t ssd[3], stray;
	uint8_t cbf_chroma[2][256];
	int16_t adi[264], adi_f[264];
	uint8_t pred[2][1024];
	int16_t lv[2][1024], rec[2][1024];
} hmr_gpu_helper_out;
int hmr_gpu_walk_helper_forms(const hmr_gpu_helper_case *cases, int ncases, const uint8_t *arena, size_t arena_bytes, hmr_gpu_helper_out *out);

/* ------------------------------------------------------------------------------------------------
 * 19. Test aid: the merge evaluation of an 8 x 8 or 16 x 16 CU as the device runs it, and the device-only body of motion_compensate_cu
 *     For these CUs check_rd_cost_merge (homerhevc_amd/csrc/enc/enc_ctu.h) does not run its candidate loop on the device: quad_load_cands -> quad_prepare (every distinct
 *     candidate side by side: luma on the worker, chroma on the helper through HJOB_QUAD_C) -> quad_merge_loop (the loop replayed on figures in registers) -> quad_commit
 *     (one deferred write of the windows of two depths, the per-depth buffers, the CTU's record, the prediction window, Enc::inter_ssq and the node), enc/enc_quad.h.
 *     Section 16 pins the tiles' arithmetic; this entry pins the replay and the commit, and motion_compensate_cu's three-block fetch from the phase planes
 *     (tests/test_gpu_merge_forms.py).  It follows section 18's rules: workgroups of a worker wavefront and its real helper wavefront, the pool kernel's LDS places and
 *     register budget, entered through rows_enter and left through release_helpers, group types of the harness's own; no wait loop of its own (it waits inside
 *     quad_prepare and helper_wait only), no way out of the worker's loop over its cases but its end.  One CtuPublic in HBM per workgroup is Enc::ctu.  Host pointers,
 *     synchronous, default context: one upload, one launch, one download per call.
 *     arena: curr, pred (6144 bytes each: the worker's source / prediction windows as in section 16; multiples of 4) and the phase planes behind sub_y / sub_c in the
 *     addressing of section 16, row pitches stride_y / stride_c.
 *     Before every step each 32-bit word of the workgroup's WorkSlow and of its CtuPublic holds 0x12341234 (a byte array of the record that starts at an even offset
 *     holds 0x34 at even entries, 0x12 at odd ones).
 *     Step MERGE (node: an 8 x 8 or 16 x 16 CU; `units`: its size * size / 16 4 x 4 units from Geo::abs_index on, depth = 3 or 2):
 *       filled from the case: the windows, Work::merge_cands (mv, ref_idx), inter_modes, Seq (width, height, margin_y = margin, stride_y, stride_c, perf_mode,
 *       sign_hiding, chroma_qp_offset), FrameCtx (slice_type P, avg_dist, chroma_weight, sub_y, sub_c), the node's qp;
 *       planted: every other byte of the node 0xEE, then Node::inter_ref_index = old_ref_index; Work::intra_mode_buffs[k][depth][unit u] = 0x40 + 0x20 k + (u & 15);
 *       Work::cbf_buffs[0..2][depth][units] and Work::tr_idx_buffs[depth][units] = 0x77; CtuPublic::cbf[k][units] = 0xa0 + k; Enc::inter_ssq[] = 0xEEEEEEEE,
 *       Enc::inter_ssq_valid = -1; the prediction window = pred;
 *       then HJOB_NEW_CTU, and the three statements of check_rd_cost_merge: quad_load_cands; quad_prepare<8 | 16>; if (slots >= 0) quad_merge_loop<8 | 16>.
 *       out: slots (quad_prepare's return value: -1, or the slot of candidate k in bits 4 k .. 4 k + 3), ret (quad_merge_loop's), the node's fields, Enc::inter_ssq /
 *       inter_ssq_valid, the per-depth buffers and the record's arrays over the units (entry u: unit abs_index + u; entries behind the CU's units are 0), lv / dec: the
 *       level and the decoded windows of [0] depth + 1 and [1] window 0 - the Y block row by row, then U, then V (an 8 x 8 CU: 64 + 16 + 16 entries, the rest 0) -, pred:
 *       the whole prediction window after the step, pred_rest: the sum of (i + 1) x byte i over the bytes of that window OUTSIDE the CU's three blocks, modulo 2^32.
 *       quad_prepare returns -1 and nothing runs behind it (performance_mode 0; a candidate whose block leaves the padded picture - quirk Q12): everything above then
 *       holds what was planted.
 *     Step MC (node: a CU of 8, 16, 32 or 64): motion_compensate_cu(node, mv[0]) on the prediction window `pred`.  out: pred, pred_rest.
 *     stray (both steps): after the harness has put 0x12341234 back over the CU's blocks of the four windows and over the record's cbf / tr_idx / intra_mode / mv_ref_idx
 *     entries of the CU's units, the number of 32-bit words of WorkSlow and CtuPublic that hold anything else.  cand_* / n_stale_pred are not written by this entry
 *     (the one-lane twin of this step, oracle/enc_cpu.cpp henc_cpu_merge_cases, reports the candidate list it derived there).
 *     Refused with HMR_GPU_ERR_ARG and a text (hmr_gpu_last_error) before anything is launched: "step"; "step (the library was built with a helper per chroma plane)"
 *     (HENC_NHELP = 2: every step); "step (the library was built without the merge tiles)" (MERGE); "node"; "node (MERGE: an 8 x 8 or 16 x 16 CU)"; "node (MC: a CU of
 *     8 to 64)"; "qp"; "perf_mode"; "chroma_qp_offset"; "sign_hiding"; "avg_dist / chroma_weight"; "ctu_x / ctu_y"; "width / height / margin"; "stride"; "reserved";
 *     "mv"; "ref_idx"; "inter_modes"; "old_ref_index"; "curr"; "pred"; "a luma prediction block outside the arena"; "a chroma prediction block outside the arena".
 * ------------------------------------------------------------------------------------------------ */
enum hmr_gpu_merge_step { HMR_GPU_MERGE_MERGE = 1, HMR_GPU_MERGE_MC };
typedef struct hmr_gpu_merge_case {
	int32_t step, node, qp, perf_mode;
	int32_t ctu_x, ctu_y, width, height;
	int32_t margin, stride_y, stride_c, sign_hiding;
	int32_t chroma_qp_offset, old_ref_index, reserved[2];      /* reserved: 0 */
	int32_t mv[2][2], ref_idx[2], inter_modes[2];               /* the candidate list: x, y in quarter samples; MC: mv[0] */
	double avg_dist, chroma_weight;
	int64_t sub_y, sub_c[2], curr, pred;
} hmr_gpu_merge_case;      /* 152 bytes */
typedef struct hmr_gpu_merge_out {
	int32_t slots;
	uint32_t ret;
	int32_t skipped, inter_mv[2], inter_ref_index;
	uint32_t cost, distortion;
	int32_t merge_flag, merge_idx, inter_mode;
	uint32_t sum;
	int32_t inter_cbf[3], inter_tr_idx;
	uint32_t inter_ssq[3];
	int32_t inter_ssq_valid;
	uint32_t stray, pred_rest;
	int32_t cand_mv[2][2], cand_ref[2], cand_modes[2], n_stale_pred;
	uint32_t reserved;
	uint8_t cbf_buffs[3][16], tr_idx_buffs[16];
	uint8_t rec_cbf[3][16], rec_tr_idx[16], rec_intra_mode[2][16];
	int8_t rec_mv_ref_idx[16];
	int16_t lv[2][384], dec[2][384];
	uint8_t pred[6144];
} hmr_gpu_merge_out;       /* 9520 bytes */
int hmr_gpu_walk_merge_forms(const hmr_gpu_merge_case *cases, int ncases, const uint8_t *arena, size_t arena_bytes, hmr_gpu_merge_out *out);

#ifdef __cplusplus
}
#endif
#endif /* HOMER_GPU_H */
