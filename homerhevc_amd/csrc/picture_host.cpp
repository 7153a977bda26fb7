// Picture conversion, the part that runs on the host alone (include/homer_gpu.h sections 12d .. 12l): the builders of the kernels' jobs (picture_io.h), the three
// descriptor checks, the host twins of the kernels - the loops a caller would write from the arithmetic headers (rgb_yuv.h, yuv_depth.h, scale_area.h, yuv_rgb.h,
// ssim_window.h, cut_stats.h), compiled from the very functions the kernels of picture_io.hip compile - and the metric arithmetic on the kernels' sums.  Nothing here touches a device.
#include <math.h>
#include <string.h>
#include "picture_io.h"

// ---- the jobs ----
IngestJob hmr_ingest_job(const hmr_gpu_picture &pic, int16_t *const dst[3], int stride_y, int stride_c, int width, int height)
{
	IngestJob j;
	hmr_job_planes(j, pic, dst, stride_y, stride_c);
	j.width = width; j.height = height;
	j.format = pic.format; j.reserved = 0;
	return j;
}

RgbIngestJob hmr_rgb_ingest_job(const hmr_gpu_rgb_picture &pic, int16_t *const dst[3], int stride_y, int stride_c, int width, int height)
{
	RgbIngestJob j;
	memset(&j, 0, sizeof j);
	hmr_rgb_source(j, pic, dst, stride_y, stride_c);
	j.width = width; j.height = height;
	return j;
}

YuvIngestJob hmr_yuv_ingest_job(const hmr_gpu_yuv_picture &pic, int16_t *const dst[3], int stride_y, int stride_c, int width, int height)
{
	YuvIngestJob j;
	memset(&j, 0, sizeof j);
	hmr_job_planes(j, pic, dst, stride_y, stride_c);
	j.width = width; j.height = height;
	j.f = hmr_yuv_form(pic.format, pic.chroma, pic.bits, pic.msb_aligned, pic.offset);
	return j;
}

EgressJob hmr_egress_job(int16_t *const rec[3], int stride_y, int stride_c, const hmr_gpu_picture *pic, int16_t *const src[3], int src_stride_y, int src_stride_c, uint64_t *ssd,
			 int width, int height)
{
	EgressJob j;
	for (int c = 0; c < 3; c++) {
		j.rec[c] = rec[c];
		j.src[c] = src ? src[c] : nullptr;
		j.dst[c] = pic ? const_cast<uint8_t *>(pic->plane[c]) : nullptr;      // (as the output descriptor: the call writes through the plane pointers)
		j.pitch[c] = pic ? pic->pitch[c] : 0;
	}
	j.ssd = ssd;
	j.stride_y = stride_y; j.stride_c = stride_c;
	j.src_stride_y = src_stride_y; j.src_stride_c = src_stride_c;
	j.width = width; j.height = height;
	j.format = pic ? pic->format : HMR_GPU_PIC_I420; j.reserved = 0;
	return j;
}

RgbEgressJob hmr_rgb_egress_job(int16_t *const yuv[3], int stride_y, int stride_c, const hmr_gpu_rgb_picture *out, const hmr_gpu_rgb_picture *ref, uint64_t *ssd, int width, int height)
{
	RgbEgressJob j;
	memset(&j, 0, sizeof j);
	for (int c = 0; c < 3; c++) {
		j.yuv[c] = yuv[c];
		if (out) {
			j.dst[c] = (uint8_t *)const_cast<void *>(out->plane[c]);      // (as the output descriptor of 12e: the call writes through the plane pointers)
			j.dst_pitch[c] = out->pitch[c];
			j.offset[c] = out->offset[c];
		}
		if (ref) {
			j.src[c] = (const uint8_t *)ref->plane[c];
			j.pitch[c] = ref->pitch[c];
			j.src_offset[c] = ref->offset[c];
		}
	}
	j.ssd = ssd;
	j.stride_y = stride_y; j.stride_c = stride_c;
	j.width = width; j.height = height;
	j.format = out ? out->format : -1; j.pixel_bytes = out ? out->pixel_bytes : 0;
	j.src_format = ref ? ref->format : -1; j.src_pixel_bytes = ref ? ref->pixel_bytes : 0;
	const hmr_gpu_rgb_picture &colour = out ? *out : *ref;      // (sums alone: the table comes from the reference's fields)
	j.m = hmr_yuv_matrix(colour.matrix, colour.full_range);
	return j;
}

SsimJob hmr_ssim_job(int16_t *const a[3], int stride_a_y, int stride_a_c, int16_t *const b[3], int stride_b_y, int stride_b_c, int64_t *sum, int width, int height)
{
	SsimJob j;
	for (int c = 0; c < 3; c++) {
		j.a[c] = a[c];
		j.b[c] = b[c];
	}
	j.sum = sum;
	j.stride_a_y = stride_a_y; j.stride_a_c = stride_a_c;
	j.stride_b_y = stride_b_y; j.stride_b_c = stride_b_c;
	j.width = width; j.height = height;
	return j;
}

CutJob hmr_cut_job(int16_t *const cur[3], int16_t *const prev[3], int stride_y, int stride_c, int64_t *stats, uint32_t *bins, int width, int height)
{
	CutJob j;
	for (int c = 0; c < 3; c++) {
		j.cur[c] = cur[c];
		j.prev[c] = prev[c];
	}
	j.stats = stats; j.bins = bins;
	j.stride_y = stride_y; j.stride_c = stride_c;
	j.width = width; j.height = height;
	return j;
}

// ---- sections 12d and 12f: the descriptor checks and the host side of the RGB ingest ----
static int refuse(const char *what)
{
	hmr_set_error("hmr_gpu_picture: %s", what);
	return HMR_GPU_ERR_ARG;
}
// a descriptor against a picture size, on the host alone
extern "C" int hmr_gpu_picture_check(const hmr_gpu_picture *pic, int width, int height)
{
	if (!pic) return refuse("the descriptor is NULL");
	if (pic->format != HMR_GPU_PIC_I420 && pic->format != HMR_GPU_PIC_NV12) return refuse("format: neither HMR_GPU_PIC_I420 nor HMR_GPU_PIC_NV12");
	if (pic->reserved != 0) return refuse("reserved: must be 0");
	if (width <= 0 || (width & 1)) return refuse("width: must be positive and even");
	if (height <= 0 || (height & 1)) return refuse("height: must be positive and even");
	const int planes = pic->format == HMR_GPU_PIC_NV12 ? 2 : 3;
	static const char *const missing[3] = {"plane[0]: NULL", "plane[1]: NULL", "plane[2]: NULL"};
	static const char *const negative[3] = {"pitch[0]: negative", "pitch[1]: negative", "pitch[2]: negative"};
	static const char *const narrow[3] = {"pitch[0]: less than a row's bytes (width)", "pitch[1]: less than a row's bytes (I420: width / 2, NV12: width)", "pitch[2]: less than a row's bytes (width / 2)"};
	for (int c = 0; c < planes; c++) {
		if (!pic->plane[c]) return refuse(missing[c]);
		if (pic->pitch[c] < 0) return refuse(negative[c]);
		const int row_bytes = c == 0 || pic->format == HMR_GPU_PIC_NV12 ? width : width / 2;
		if (pic->pitch[c] < row_bytes) return refuse(narrow[c]);
	}
	if (planes == 2 && pic->plane[2]) return refuse("plane[2]: must be NULL for NV12 (plane[1] holds the U, V pairs)");
	return HMR_GPU_OK;
}

static int refuse_rgb(const char *what)
{
	hmr_set_error("hmr_gpu_rgb_picture: %s", what);
	return HMR_GPU_ERR_ARG;
}
// an RGB descriptor against a picture size, on the host alone
extern "C" int hmr_gpu_rgb_picture_check(const hmr_gpu_rgb_picture *pic, int width, int height)
{
	if (!pic) return refuse_rgb("the descriptor is NULL");
	if (pic->format < HMR_GPU_RGB_PACKED8 || pic->format > HMR_GPU_RGB_PLANAR_F32) return refuse_rgb("format: not one of HMR_GPU_RGB_PACKED8, _PLANAR8, _PLANAR_F16, _PLANAR_F32");
	if (pic->matrix != HMR_GPU_MATRIX_BT601 && pic->matrix != HMR_GPU_MATRIX_BT709) return refuse_rgb("matrix: neither HMR_GPU_MATRIX_BT601 nor HMR_GPU_MATRIX_BT709");
	if (pic->full_range != 0 && pic->full_range != 1) return refuse_rgb("full_range: must be 0 or 1");
	if (pic->reserved != 0) return refuse_rgb("reserved: must be 0");
	if (width <= 0 || (width & 1)) return refuse_rgb("width: must be positive and even");
	if (height <= 0 || (height & 1)) return refuse_rgb("height: must be positive and even");
	const bool packed = pic->format == HMR_GPU_RGB_PACKED8;
	static const char *const offset_range[3] = {"offset[0]: outside 0 .. pixel_bytes - 1", "offset[1]: outside 0 .. pixel_bytes - 1", "offset[2]: outside 0 .. pixel_bytes - 1"};
	static const char *const offset_zero[3] = {"offset[0]: must be 0 for a planar format", "offset[1]: must be 0 for a planar format", "offset[2]: must be 0 for a planar format"};
	if (packed) {
		if (pic->pixel_bytes != 3 && pic->pixel_bytes != 4) return refuse_rgb("pixel_bytes: must be 3 or 4 for HMR_GPU_RGB_PACKED8");
		for (int c = 0; c < 3; c++)
			if (pic->offset[c] < 0 || pic->offset[c] >= pic->pixel_bytes) return refuse_rgb(offset_range[c]);
		if (pic->offset[1] == pic->offset[0]) return refuse_rgb("offset[1]: the same byte as offset[0]");
		if (pic->offset[2] == pic->offset[0] || pic->offset[2] == pic->offset[1]) return refuse_rgb("offset[2]: the same byte as another channel's");
	} else {
		if (pic->pixel_bytes != 0) return refuse_rgb("pixel_bytes: must be 0 for a planar format");
		for (int c = 0; c < 3; c++)
			if (pic->offset[c] != 0) return refuse_rgb(offset_zero[c]);
	}
	const int elem = packed ? pic->pixel_bytes : pic->format == HMR_GPU_RGB_PLANAR8 ? 1 : pic->format == HMR_GPU_RGB_PLANAR_F16 ? 2 : 4;
	const int align = packed ? 1 : elem;
	static const char *const missing[3] = {"plane[0]: NULL", "plane[1]: NULL", "plane[2]: NULL"};
	static const char *const extra[3] = {"", "plane[1]: must be NULL for HMR_GPU_RGB_PACKED8 (plane[0] holds the pixels)", "plane[2]: must be NULL for HMR_GPU_RGB_PACKED8 (plane[0] holds the pixels)"};
	static const char *const negative[3] = {"pitch[0]: negative", "pitch[1]: negative", "pitch[2]: negative"};
	static const char *const narrow[3] = {"pitch[0]: less than a row's bytes (width x pixel_bytes, or width x the element size)", "pitch[1]: less than a row's bytes (width x the element size)",
					      "pitch[2]: less than a row's bytes (width x the element size)"};
	static const char *const plane_align[3] = {"plane[0]: not a multiple of the element size", "plane[1]: not a multiple of the element size", "plane[2]: not a multiple of the element size"};
	static const char *const pitch_align[3] = {"pitch[0]: not a multiple of the element size", "pitch[1]: not a multiple of the element size", "pitch[2]: not a multiple of the element size"};
	for (int c = 0; c < 3; c++) {
		if (packed && c) {
			if (pic->plane[c]) return refuse_rgb(extra[c]);
			continue;
		}
		if (!pic->plane[c]) return refuse_rgb(missing[c]);
		if (pic->pitch[c] < 0) return refuse_rgb(negative[c]);
		if (pic->pitch[c] < (int64_t)width * elem) return refuse_rgb(narrow[c]);
		if ((uintptr_t)pic->plane[c] % align) return refuse_rgb(plane_align[c]);
		if (pic->pitch[c] % align) return refuse_rgb(pitch_align[c]);
	}
	return HMR_GPU_OK;
}

// rgb_yuv.h's arithmetic over host memory: the loop a caller would write from the header's formulas
extern "C" int hmr_gpu_rgb_convert_host(const hmr_gpu_rgb_picture *pic, int width, int height, uint8_t *y, uint8_t *u, uint8_t *v)
{
	const int rc = hmr_gpu_rgb_picture_check(pic, width, height);
	if (rc) return rc;
	if (!y || !u || !v) {
		hmr_set_error("hmr_gpu_rgb_convert_host: needs the three output planes");
		return HMR_GPU_ERR_ARG;
	}
	const RgbMatrix m = hmr_rgb_matrix(pic->matrix, pic->full_range);
	const bool packed = pic->format == HMR_GPU_RGB_PACKED8;
	for (int by = 0; by < height; by += 2)
		for (int bx = 0; bx < width; bx += 2) {
			int s[3] = {0, 0, 0};
			for (int k = 0; k < 4; k++) {
				const int px = bx + (k & 1), py = by + (k >> 1);
				int c3[3];
				for (int c = 0; c < 3; c++) {
					c3[c] = rgb_sample<const uint8_t *, const _Float16 *, const float *>((const uint8_t *)pic->plane[packed ? 0 : c], pic->pitch[packed ? 0 : c], pic->format, pic->pixel_bytes,
													      pic->offset[c], px, py);
					s[c] += c3[c];
				}
				y[(size_t)py * width + px] = (uint8_t)hmr_rgb_luma(m, c3[0], c3[1], c3[2]);
			}
			const size_t oc = (size_t)(by >> 1) * (width >> 1) + (bx >> 1);
			u[oc] = (uint8_t)hmr_rgb_chroma(m.u, s[0], s[1], s[2]);
			v[oc] = (uint8_t)hmr_rgb_chroma(m.v, s[0], s[1], s[2]);
		}
	return HMR_GPU_OK;
}

// ---- section 12k: the host side of the deep / 4:2:2 / 4:4:4 ingest ----
static_assert(HMR_YUV_PLANAR == HMR_GPU_YUV_PLANAR && HMR_YUV_SEMIPLANAR == HMR_GPU_YUV_SEMIPLANAR && HMR_YUV_PACKED422 == HMR_GPU_YUV_PACKED422, "yuv_depth.h restates the header's formats");
static int refuse_yuv(const char *what)
{
	hmr_set_error("hmr_gpu_yuv_picture: %s", what);
	return HMR_GPU_ERR_ARG;
}
// a Y'CbCr descriptor against a picture size, on the host alone
extern "C" int hmr_gpu_yuv_picture_check(const hmr_gpu_yuv_picture *pic, int width, int height)
{
	if (!pic) return refuse_yuv("the descriptor is NULL");
	if (pic->format < HMR_GPU_YUV_PLANAR || pic->format > HMR_GPU_YUV_PACKED422) return refuse_yuv("format: not one of HMR_GPU_YUV_PLANAR, _SEMIPLANAR, _PACKED422");
	if (pic->chroma < HMR_GPU_CHROMA_420 || pic->chroma > HMR_GPU_CHROMA_444) return refuse_yuv("chroma: not one of HMR_GPU_CHROMA_420, _422, _444");
	if (pic->bits < 8 || pic->bits > 16) return refuse_yuv("bits: outside 8 .. 16");
	if (pic->msb_aligned != 0 && pic->msb_aligned != 1) return refuse_yuv("msb_aligned: must be 0 or 1");
	if (pic->msb_aligned && (pic->bits == 8 || pic->bits == 16)) return refuse_yuv("msb_aligned: must be 0 with bits 8 or 16 (the sample fills its container)");
	if (pic->reserved != 0) return refuse_yuv("reserved: must be 0");
	if (width <= 0 || (width & 1)) return refuse_yuv("width: must be positive and even");
	if (height <= 0 || (height & 1)) return refuse_yuv("height: must be positive and even");
	if (pic->format == HMR_GPU_YUV_PACKED422 && pic->chroma != HMR_GPU_CHROMA_422) return refuse_yuv("chroma: must be HMR_GPU_CHROMA_422 for HMR_GPU_YUV_PACKED422");
	static const char *const offset_zero[3] = {"offset[0]: must be 0 for this format", "offset[1]: must be 0 for HMR_GPU_YUV_PLANAR", "offset[2]: must be 0 for HMR_GPU_YUV_PLANAR"};
	if (pic->format == HMR_GPU_YUV_PLANAR) {
		for (int c = 0; c < 3; c++)
			if (pic->offset[c] != 0) return refuse_yuv(offset_zero[c]);
	} else if (pic->format == HMR_GPU_YUV_SEMIPLANAR) {
		if (pic->offset[0] != 0) return refuse_yuv(offset_zero[0]);
		if (pic->offset[1] < 0 || pic->offset[1] > 1) return refuse_yuv("offset[1]: outside 0 .. 1 (U's place in a pair)");
		if (pic->offset[2] < 0 || pic->offset[2] > 1) return refuse_yuv("offset[2]: outside 0 .. 1 (V's place in a pair)");
		if (pic->offset[2] == pic->offset[1]) return refuse_yuv("offset[2]: the same sample of a pair as offset[1]");
	} else {
		if (pic->offset[0] < 0 || pic->offset[0] > 1) return refuse_yuv("offset[0]: outside 0 .. 1 (the first luma sample of a group of four)");
		if (pic->offset[1] < 0 || pic->offset[1] > 3) return refuse_yuv("offset[1]: outside 0 .. 3");
		if (pic->offset[2] < 0 || pic->offset[2] > 3) return refuse_yuv("offset[2]: outside 0 .. 3");
		if (((pic->offset[1] ^ pic->offset[0]) & 1) == 0) return refuse_yuv("offset[1]: a luma sample's place (offset[0] and offset[0] + 2)");
		if (((pic->offset[2] ^ pic->offset[0]) & 1) == 0) return refuse_yuv("offset[2]: a luma sample's place (offset[0] and offset[0] + 2)");
		if (pic->offset[2] == pic->offset[1]) return refuse_yuv("offset[2]: the same sample of a group as offset[1]");
	}
	const int planes = pic->format == HMR_GPU_YUV_PLANAR ? 3 : pic->format == HMR_GPU_YUV_SEMIPLANAR ? 2 : 1;
	const int sb = pic->bits > 8 ? 2 : 1;
	const int64_t wc = pic->chroma == HMR_GPU_CHROMA_444 ? width : width / 2;
	const int64_t row_bytes[3] = {(pic->format == HMR_GPU_YUV_PACKED422 ? 2 : 1) * (int64_t)width * sb, (pic->format == HMR_GPU_YUV_SEMIPLANAR ? 2 : 1) * wc * sb, wc * sb};
	static const char *const missing[3] = {"plane[0]: NULL", "plane[1]: NULL", "plane[2]: NULL"};
	static const char *const extra[3] = {"", "plane[1]: must be NULL for HMR_GPU_YUV_PACKED422 (plane[0] holds the samples)", "plane[2]: must be NULL for this format (it has no third plane)"};
	static const char *const negative[3] = {"pitch[0]: negative", "pitch[1]: negative", "pitch[2]: negative"};
	static const char *const narrow[3] = {"pitch[0]: less than a row's bytes (W sb; PACKED422: 2 W sb)", "pitch[1]: less than a row's bytes (Wc sb; SEMIPLANAR: 2 Wc sb)", "pitch[2]: less than a row's bytes (Wc sb)"};
	static const char *const plane_align[3] = {"plane[0]: not a multiple of 2 (16-bit containers)", "plane[1]: not a multiple of 2 (16-bit containers)", "plane[2]: not a multiple of 2 (16-bit containers)"};
	static const char *const pitch_align[3] = {"pitch[0]: not a multiple of 2 (16-bit containers)", "pitch[1]: not a multiple of 2 (16-bit containers)", "pitch[2]: not a multiple of 2 (16-bit containers)"};
	for (int c = 0; c < 3; c++) {
		if (c >= planes) {
			if (pic->plane[c]) return refuse_yuv(extra[c]);
			continue;
		}
		if (!pic->plane[c]) return refuse_yuv(missing[c]);
		if (pic->pitch[c] < 0) return refuse_yuv(negative[c]);
		if (pic->pitch[c] < row_bytes[c]) return refuse_yuv(narrow[c]);
		if ((uintptr_t)pic->plane[c] % sb) return refuse_yuv(plane_align[c]);
		if (pic->pitch[c] % sb) return refuse_yuv(pitch_align[c]);
	}
	return HMR_GPU_OK;
}

// yuv_depth.h's arithmetic over host memory: the loop a caller would write from the header's formulas
extern "C" int hmr_gpu_yuv_convert_host(const hmr_gpu_yuv_picture *pic, int width, int height, uint8_t *y, uint8_t *u, uint8_t *v)
{
	const int rc = hmr_gpu_yuv_picture_check(pic, width, height);
	if (rc) return rc;
	if (!y || !u || !v) {
		hmr_set_error("hmr_gpu_yuv_convert_host: needs the three output planes");
		return HMR_GPU_ERR_ARG;
	}
	const YuvForm f = hmr_yuv_form(pic->format, pic->chroma, pic->bits, pic->msb_aligned, pic->offset);
	for (int py = 0; py < height; py++)
		for (int px = 0; px < width; px++) y[(size_t)py * width + px] = (uint8_t)hmr_yuv_luma<const uint8_t *>(pic->plane, pic->pitch, f, px, py);
	for (int cy = 0; cy < height / 2; cy++)
		for (int cx = 0; cx < width / 2; cx++) {
			u[(size_t)cy * (width / 2) + cx] = (uint8_t)hmr_yuv_chroma<const uint8_t *>(pic->plane, pic->pitch, f, 1, cx, cy);
			v[(size_t)cy * (width / 2) + cx] = (uint8_t)hmr_yuv_chroma<const uint8_t *>(pic->plane, pic->pitch, f, 2, cx, cy);
		}
	return HMR_GPU_OK;
}

// ---- section 12g: the host side of the downscaling ingest ----
extern "C" int hmr_gpu_scale_check(int src_w, int src_h, int dst_w, int dst_h)
{
	const char *why = hmr_scale_refusal(src_w, src_h, dst_w, dst_h);
	if (!why) return HMR_GPU_OK;
	hmr_set_error("hmr_gpu_scale_check: %d x %d -> %d x %d: %s", src_w, src_h, dst_w, dst_h, why);
	return HMR_GPU_ERR_ARG;
}

// scale_area.h's arithmetic over host memory: the loop a caller would write from the header's formula
extern "C" int hmr_gpu_scale_host(const hmr_gpu_scaled_picture *pic, int dst_w, int dst_h, uint8_t *y, uint8_t *u, uint8_t *v)
{
	if (!pic) {
		hmr_set_error("hmr_gpu_scale_host: the descriptor is NULL");
		return HMR_GPU_ERR_ARG;
	}
	const int rc = hmr_gpu_picture_check(&pic->pic, pic->width, pic->height);
	if (rc) return rc;
	if (const char *why = hmr_scale_refusal(pic->width, pic->height, dst_w, dst_h, true)) {      // (any ratio: the bound of 8 is the kernel's)
		hmr_set_error("hmr_gpu_scale_host: %d x %d -> %d x %d: %s", pic->width, pic->height, dst_w, dst_h, why);
		return HMR_GPU_ERR_ARG;
	}
	if (!y || !u || !v) {
		hmr_set_error("hmr_gpu_scale_host: needs the three output planes");
		return HMR_GPU_ERR_ARG;
	}
	const hmr_gpu_picture &p = pic->pic;
	const int ws = pic->width, hs = pic->height;
	hmr_scale_plane_host(p.plane[0], p.pitch[0], 1, ws, hs, dst_w, dst_h, y);
	if (p.format == HMR_GPU_PIC_NV12) {
		hmr_scale_plane_host(p.plane[1], p.pitch[1], 2, ws / 2, hs / 2, dst_w / 2, dst_h / 2, u);
		hmr_scale_plane_host(p.plane[1] + 1, p.pitch[1], 2, ws / 2, hs / 2, dst_w / 2, dst_h / 2, v);
	} else {
		hmr_scale_plane_host(p.plane[1], p.pitch[1], 1, ws / 2, hs / 2, dst_w / 2, dst_h / 2, u);
		hmr_scale_plane_host(p.plane[2], p.pitch[2], 1, ws / 2, hs / 2, dst_w / 2, dst_h / 2, v);
	}
	return HMR_GPU_OK;
}

// ---- section 12j: the host side of the downscaling RGB ingest ----
// rgb_yuv.h's and scale_area.h's arithmetic over host memory, the loop a caller would write from section 12j: every output sums its taps, and each tap converts the
// pixel (luma) or the 2 x 2 block (chroma) it stands on; no converted picture in between
extern "C" int hmr_gpu_scale_rgb_host(const hmr_gpu_scaled_rgb_picture *pic, int dst_w, int dst_h, uint8_t *y, uint8_t *u, uint8_t *v)
{
	if (!pic) {
		hmr_set_error("hmr_gpu_scale_rgb_host: the descriptor is NULL");
		return HMR_GPU_ERR_ARG;
	}
	const int rc = hmr_gpu_rgb_picture_check(&pic->pic, pic->width, pic->height);
	if (rc) return rc;
	if (const char *why = hmr_scale_refusal(pic->width, pic->height, dst_w, dst_h, true)) {      // (any ratio: the bound of 8 is the kernel's)
		hmr_set_error("hmr_gpu_scale_rgb_host: %d x %d -> %d x %d: %s", pic->width, pic->height, dst_w, dst_h, why);
		return HMR_GPU_ERR_ARG;
	}
	if (!y || !u || !v) {
		hmr_set_error("hmr_gpu_scale_rgb_host: needs the three output planes");
		return HMR_GPU_ERR_ARG;
	}
	const hmr_gpu_rgb_picture &p = pic->pic;
	const RgbMatrix m = hmr_rgb_matrix(p.matrix, p.full_range);
	const bool packed = p.format == HMR_GPU_RGB_PACKED8;
	const ScaleAxis ax = hmr_scale_axis(pic->width, dst_w), ay = hmr_scale_axis(pic->height, dst_h);      // (a chroma axis has the same reduced ratio)
	const uint32_t den = ax.s * ay.s;
	auto sample = [&](int c, int px, int py) {
		return rgb_sample<const uint8_t *, const _Float16 *, const float *>((const uint8_t *)p.plane[packed ? 0 : c], p.pitch[packed ? 0 : c], p.format, p.pixel_bytes, p.offset[c], px, py);
	};
	for (int oy = 0; oy < dst_h; oy++)
		for (int ox = 0; ox < dst_w; ox++) {
			uint32_t sum = den >> 1;
			for (uint32_t sj = (uint32_t)oy * ay.s / ay.d; sj * ay.d < ((uint32_t)oy + 1) * ay.s; sj++)
				for (uint32_t si = (uint32_t)ox * ax.s / ax.d; si * ax.d < ((uint32_t)ox + 1) * ax.s; si++)
					sum += hmr_scale_weight(ay, (uint32_t)oy, sj) * hmr_scale_weight(ax, (uint32_t)ox, si) *
					       (uint32_t)hmr_rgb_luma(m, sample(0, (int)si, (int)sj), sample(1, (int)si, (int)sj), sample(2, (int)si, (int)sj));
			y[(size_t)oy * dst_w + ox] = (uint8_t)(sum / den);
		}
	for (int oy = 0; oy < dst_h / 2; oy++)
		for (int ox = 0; ox < dst_w / 2; ox++) {
			uint32_t sum_u = den >> 1, sum_v = den >> 1;
			for (uint32_t sj = (uint32_t)oy * ay.s / ay.d; sj * ay.d < ((uint32_t)oy + 1) * ay.s; sj++)
				for (uint32_t si = (uint32_t)ox * ax.s / ax.d; si * ax.d < ((uint32_t)ox + 1) * ax.s; si++) {
					int s[3] = {0, 0, 0};      // the sums of the 2 x 2 block under source chroma sample (si, sj)
					for (int k = 0; k < 4; k++)
						for (int c = 0; c < 3; c++) s[c] += sample(c, 2 * (int)si + (k & 1), 2 * (int)sj + (k >> 1));
					const uint32_t w = hmr_scale_weight(ay, (uint32_t)oy, sj) * hmr_scale_weight(ax, (uint32_t)ox, si);
					sum_u += w * (uint32_t)hmr_rgb_chroma(m.u, s[0], s[1], s[2]);
					sum_v += w * (uint32_t)hmr_rgb_chroma(m.v, s[0], s[1], s[2]);
				}
			const size_t oc = (size_t)oy * (dst_w / 2) + ox;
			u[oc] = (uint8_t)(sum_u / den);
			v[oc] = (uint8_t)(sum_v / den);
		}
	return HMR_GPU_OK;
}

// ---- section 12l: the host side of the downscaling deep / 4:2:2 / 4:4:4 ingest ----
// yuv_depth.h's and scale_area.h's arithmetic over host memory, the loop a caller would write from section 12l: every output sums its taps, and each tap rounds the
// container (luma) or the 1, 2 or 4 containers (chroma) it stands on; no converted picture in between
extern "C" int hmr_gpu_scale_yuv_host(const hmr_gpu_scaled_yuv_picture *pic, int dst_w, int dst_h, uint8_t *y, uint8_t *u, uint8_t *v)
{
	if (!pic) {
		hmr_set_error("hmr_gpu_scale_yuv_host: the descriptor is NULL");
		return HMR_GPU_ERR_ARG;
	}
	const int rc = hmr_gpu_yuv_picture_check(&pic->pic, pic->width, pic->height);
	if (rc) return rc;
	if (const char *why = hmr_scale_refusal(pic->width, pic->height, dst_w, dst_h, true)) {      // (any ratio: the bound of 8 is the kernel's)
		hmr_set_error("hmr_gpu_scale_yuv_host: %d x %d -> %d x %d: %s", pic->width, pic->height, dst_w, dst_h, why);
		return HMR_GPU_ERR_ARG;
	}
	if (!y || !u || !v) {
		hmr_set_error("hmr_gpu_scale_yuv_host: needs the three output planes");
		return HMR_GPU_ERR_ARG;
	}
	const hmr_gpu_yuv_picture &p = pic->pic;
	const YuvForm f = hmr_yuv_form(p.format, p.chroma, p.bits, p.msb_aligned, p.offset);
	const ScaleAxis ax = hmr_scale_axis(pic->width, dst_w), ay = hmr_scale_axis(pic->height, dst_h);      // (a chroma axis has the same reduced ratio)
	const uint32_t den = ax.s * ay.s;
	for (int oy = 0; oy < dst_h; oy++)
		for (int ox = 0; ox < dst_w; ox++) {
			uint32_t sum = den >> 1;
			for (uint32_t sj = (uint32_t)oy * ay.s / ay.d; sj * ay.d < ((uint32_t)oy + 1) * ay.s; sj++)
				for (uint32_t si = (uint32_t)ox * ax.s / ax.d; si * ax.d < ((uint32_t)ox + 1) * ax.s; si++)
					sum += hmr_scale_weight(ay, (uint32_t)oy, sj) * hmr_scale_weight(ax, (uint32_t)ox, si) * hmr_yuv_luma<const uint8_t *>(p.plane, p.pitch, f, (int)si, (int)sj);
			y[(size_t)oy * dst_w + ox] = (uint8_t)(sum / den);
		}
	for (int oy = 0; oy < dst_h / 2; oy++)
		for (int ox = 0; ox < dst_w / 2; ox++) {
			uint32_t sum_u = den >> 1, sum_v = den >> 1;
			for (uint32_t sj = (uint32_t)oy * ay.s / ay.d; sj * ay.d < ((uint32_t)oy + 1) * ay.s; sj++)
				for (uint32_t si = (uint32_t)ox * ax.s / ax.d; si * ax.d < ((uint32_t)ox + 1) * ax.s; si++) {
					const uint32_t w = hmr_scale_weight(ay, (uint32_t)oy, sj) * hmr_scale_weight(ax, (uint32_t)ox, si);
					sum_u += w * hmr_yuv_chroma<const uint8_t *>(p.plane, p.pitch, f, 1, (int)si, (int)sj);      // (converted chroma sample (si, sj): its 1, 2 or 4 taps)
					sum_v += w * hmr_yuv_chroma<const uint8_t *>(p.plane, p.pitch, f, 2, (int)si, (int)sj);
				}
			const size_t oc = (size_t)oy * (dst_w / 2) + ox;
			u[oc] = (uint8_t)(sum_u / den);
			v[oc] = (uint8_t)(sum_v / den);
		}
	return HMR_GPU_OK;
}

// homer_psnr's arithmetic (hmr_metics.c:66-104) on sums of squared differences: pure host
extern "C" int hmr_gpu_psnr(const uint64_t ssd[3], int width, int height, double psnr[3])
{
	if (!ssd || !psnr || width <= 0 || height <= 0 || (width & 1) || (height & 1)) {
		hmr_set_error("hmr_gpu_psnr: needs three sums, three results and a positive even width and height (%d x %d)", width, height);
		return HMR_GPU_ERR_ARG;
	}
	for (int c = 0; c < 3; c++) {
		const double samples = c ? (double)(width / 2) * (height / 2) : (double)width * height;
		psnr[c] = ssd[c] ? 10.0 * log10(255.0 * 255.0 * samples / (double)ssd[c]) : 99.99;
	}
	return HMR_GPU_OK;
}

// ---- section 12i: the host side of the RGB egress ----
// yuv_rgb.h's arithmetic over host memory: the loop a caller would write from the header's formulas
extern "C" int hmr_gpu_rgb_from_yuv_host(const uint8_t *y, const uint8_t *u, const uint8_t *v, int width, int height, const hmr_gpu_rgb_picture *out)
{
	const int rc = hmr_gpu_rgb_picture_check(out, width, height);
	if (rc) return rc;
	if (!y || !u || !v) {
		hmr_set_error("hmr_gpu_rgb_from_yuv_host: needs the three input planes");
		return HMR_GPU_ERR_ARG;
	}
	const YuvMatrix m = hmr_yuv_matrix(out->matrix, out->full_range);
	const bool packed = out->format == HMR_GPU_RGB_PACKED8;
	const int cw = width >> 1, ch = height >> 1;
	for (int py = 0; py < height; py++)
		for (int px = 0; px < width; px++) {
			int c3[3];
			hmr_yuv_rgb(m, y[(size_t)py * width + px], hmr_yuv_chroma16(u, cw, cw, ch, px, py), hmr_yuv_chroma16(v, cw, cw, ch, px, py), c3[0], c3[1], c3[2]);
			for (int c = 0; c < 3; c++)
				rgb_put<uint8_t *, _Float16 *, float *>((uint8_t *)const_cast<void *>(out->plane[packed ? 0 : c]), out->pitch[packed ? 0 : c], out->format, out->pixel_bytes, out->offset[c], px, py, c3[c]);
			if (packed && out->pixel_bytes == 4) ((uint8_t *)const_cast<void *>(out->plane[0]))[(int64_t)py * out->pitch[0] + 4 * px + rgb_alpha_offset(out->offset)] = 255;
		}
	return HMR_GPU_OK;
}

// the three sums of squared differences between the 8-bit values of two RGB pictures in host memory
extern "C" int hmr_gpu_rgb_ssd_host(const hmr_gpu_rgb_picture *a, const hmr_gpu_rgb_picture *b, int width, int height, uint64_t ssd[3])
{
	int rc;
	if ((rc = hmr_gpu_rgb_picture_check(a, width, height)) || (rc = hmr_gpu_rgb_picture_check(b, width, height))) return rc;
	if (!ssd) {
		hmr_set_error("hmr_gpu_rgb_ssd_host: needs the three sums");
		return HMR_GPU_ERR_ARG;
	}
	const hmr_gpu_rgb_picture *pics[2] = {a, b};
	for (int c = 0; c < 3; c++) {
		uint64_t sum = 0;
		for (int py = 0; py < height; py++)
			for (int px = 0; px < width; px++) {
				int s[2];
				for (int k = 0; k < 2; k++) {
					const hmr_gpu_rgb_picture *p = pics[k];
					const int plane = p->format == HMR_GPU_RGB_PACKED8 ? 0 : c;
					s[k] = rgb_sample<const uint8_t *, const _Float16 *, const float *>((const uint8_t *)p->plane[plane], p->pitch[plane], p->format, p->pixel_bytes, p->offset[c], px, py);
				}
				sum += (uint64_t)((s[0] - s[1]) * (s[0] - s[1]));
			}
		ssd[c] = sum;
	}
	return HMR_GPU_OK;
}

// PSNR of R, G, B and of all three together from sums of squared differences: pure host
extern "C" int hmr_gpu_psnr_rgb(const uint64_t ssd[3], int width, int height, double psnr[4])
{
	if (!ssd || !psnr || width <= 0 || height <= 0 || (width & 1) || (height & 1)) {
		hmr_set_error("hmr_gpu_psnr_rgb: needs three sums, four results and a positive even width and height (%d x %d)", width, height);
		return HMR_GPU_ERR_ARG;
	}
	const double samples = (double)width * height;
	for (int c = 0; c < 3; c++) psnr[c] = ssd[c] ? 10.0 * log10(255.0 * 255.0 * samples / (double)ssd[c]) : 99.99;
	const uint64_t all = ssd[0] + ssd[1] + ssd[2];
	psnr[3] = all ? 10.0 * log10(255.0 * 255.0 * 3.0 * samples / (double)all) : 99.99;
	return HMR_GPU_OK;
}

// ---- section 12h: the host side of SSIM ----
// the mean SSIM of each plane from its sum: pure host
extern "C" int hmr_gpu_ssim(const int64_t sums[3], int width, int height, double ssim[3])
{
	if (!sums || !ssim) {
		hmr_set_error("hmr_gpu_ssim: needs three sums and three results");
		return HMR_GPU_ERR_ARG;
	}
	if (const char *why = hmr_ssim_refusal(width, height)) {
		hmr_set_error("hmr_gpu_ssim: %d x %d: %s", width, height, why);
		return HMR_GPU_ERR_ARG;
	}
	for (int c = 0; c < 3; c++) {
		const int64_t windows = c ? hmr_ssim_windows(width / 2, height / 2) : hmr_ssim_windows(width, height);
		if (sums[c] > (windows << HMR_SSIM_ONE_BITS) || sums[c] < -(windows << HMR_SSIM_ONE_BITS)) {
			hmr_set_error("hmr_gpu_ssim: sums[%d] = %lld is outside +- 2^30 x %lld windows of a %d x %d picture", c, (long long)sums[c], (long long)windows, width, height);
			return HMR_GPU_ERR_ARG;
		}
		ssim[c] = (double)sums[c] / (double)(windows << HMR_SSIM_ONE_BITS);      // (both conversions exact below 2^53: ONE rounding)
	}
	return HMR_GPU_OK;
}

// ssim_window.h's arithmetic over host memory: the loop a caller would write from the header's definition
extern "C" int hmr_gpu_ssim_host(const hmr_gpu_picture *a, const hmr_gpu_picture *b, int width, int height, int64_t sums[3])
{
	int rc;
	if ((rc = hmr_gpu_picture_check(a, width, height)) || (rc = hmr_gpu_picture_check(b, width, height))) return rc;
	if (const char *why = hmr_ssim_refusal(width, height)) {
		hmr_set_error("hmr_gpu_ssim_host: %d x %d: %s", width, height, why);
		return HMR_GPU_ERR_ARG;
	}
	if (!sums) {
		hmr_set_error("hmr_gpu_ssim_host: needs the three sums");
		return HMR_GPU_ERR_ARG;
	}
	// plane c of a picture: its first sample, its pitch, the bytes from sample to sample
	struct View { const uint8_t *p; int64_t pitch; int step; };
	auto view = [](const hmr_gpu_picture &pic, int c) {
		if (c == 0 || pic.format == HMR_GPU_PIC_I420) return View{pic.plane[c], pic.pitch[c], 1};
		return View{pic.plane[1] + (c - 1), pic.pitch[1], 2};
	};
	for (int c = 0; c < 3; c++) {
		const View va = view(*a, c), vb = view(*b, c);
		sums[c] = hmr_ssim_plane_host(va.p, va.pitch, va.step, vb.p, vb.pitch, vb.step, c ? width / 2 : width, c ? height / 2 : height);
	}
	return HMR_GPU_OK;
}

// ---- section 12m: the host side of the scene-cut statistics ----
// cut_stats.h's arithmetic over host memory: the loops a caller would write from the header's definition
extern "C" int hmr_gpu_cut_stats_host(const hmr_gpu_picture *cur, const hmr_gpu_picture *prev, int width, int height, int64_t stats[8])
{
	int rc;
	if ((rc = hmr_gpu_picture_check(cur, width, height)) || (rc = hmr_gpu_picture_check(prev, width, height))) return rc;
	if (const char *why = hmr_cut_refusal(width, height)) {
		hmr_set_error("hmr_gpu_cut_stats_host: %d x %d: %s", width, height, why);
		return HMR_GPU_ERR_ARG;
	}
	if (!stats) {
		hmr_set_error("hmr_gpu_cut_stats_host: needs the eight values");
		return HMR_GPU_ERR_ARG;
	}
	struct View { const uint8_t *p; int64_t pitch; int step; };
	auto view = [](const hmr_gpu_picture &pic, int c) {
		if (c == 0 || pic.format == HMR_GPU_PIC_I420) return View{pic.plane[c], pic.pitch[c], 1};
		return View{pic.plane[1] + (c - 1), pic.pitch[1], 2};
	};
	for (int c = 0; c < 3; c++) {
		const View a = view(*cur, c), b = view(*prev, c);
		stats[HMR_CUT_SAD_Y + c] = hmr_cut_sad_plane_host(a.p, a.pitch, a.step, b.p, b.pitch, b.step, c ? width / 2 : width, c ? height / 2 : height);
	}
	hmr_cut_luma_host(cur->plane[0], cur->pitch[0], prev->plane[0], prev->pitch[0], width, height, stats);
	return HMR_GPU_OK;
}

// the four scores from the eight values: correctly rounded double quotients of exact integers, pure host
extern "C" int hmr_gpu_cut_score(const int64_t stats[8], int width, int height, double score[4])
{
	if (!stats || !score) {
		hmr_set_error("hmr_gpu_cut_score: needs eight values and four results");
		return HMR_GPU_ERR_ARG;
	}
	if (const char *why = hmr_cut_refusal(width, height)) {
		hmr_set_error("hmr_gpu_cut_score: %d x %d: %s", width, height, why);
		return HMR_GPU_ERR_ARG;
	}
	const int64_t samples = (int64_t)width * height, blocks = samples / 64;
	const int64_t most[HMR_CUT_VALUES] = {255 * samples, 255 * (samples / 4), 255 * (samples / 4), 2 * samples, HMR_CUT_MAX_ACT * blocks, HMR_CUT_MAX_ACT * blocks, blocks, 255 * samples};
	for (int k = 0; k < HMR_CUT_VALUES; k++)
		if (stats[k] < 0 || stats[k] > most[k]) {
			hmr_set_error("hmr_gpu_cut_score: stats[%d] = %lld is outside 0 .. %lld of a %d x %d picture", k, (long long)stats[k], (long long)most[k], width, height);
			return HMR_GPU_ERR_ARG;
		}
	if (stats[HMR_CUT_INTER] > stats[HMR_CUT_INTRA]) {
		hmr_set_error("hmr_gpu_cut_score: INTER = %lld is above INTRA = %lld", (long long)stats[HMR_CUT_INTER], (long long)stats[HMR_CUT_INTRA]);
		return HMR_GPU_ERR_ARG;
	}
	// (every operand is exact in a double: below 2^53 - 255 x 8192 x 8192 = 1.7e10 - so each quotient is rounded ONCE)
	score[0] = (double)stats[HMR_CUT_SAD_Y] / (double)samples;
	score[1] = (double)stats[HMR_CUT_HIST] / (double)(2 * samples);
	score[2] = (double)stats[HMR_CUT_NINTRA] / (double)blocks;
	score[3] = stats[HMR_CUT_INTRA] ? (double)stats[HMR_CUT_INTER] / (double)stats[HMR_CUT_INTRA] : 1.0;
	return HMR_GPU_OK;
}
