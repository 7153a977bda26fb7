// Picture conversion on the device (picture_io.hip): 8-bit 4:2:0 pictures in device memory <-> the int16 planes of the frame encoder, a batch of pictures per launch.
// Ingest: 8-bit pictures -> int16 planes (a picture slot, a reference picture); RGB pictures (8-bit packed or planar, binary16, binary32) -> the same planes, colour
// converted in the same pass (rgb_yuv.h); Y'CbCr pictures of 8 .. 16 bits in 4:2:0, 4:2:2 or 4:4:4, planar, semi-planar or packed -> the same planes, rounded to 8-bit 4:2:0 in the same pass (yuv_depth.h); 8-bit pictures of another, larger size -> the same planes, area-averaged in the same pass (scale_area.h); RGB pictures of a larger size -> the same planes, converted and area-averaged in the same pass; Y'CbCr pictures of 8 .. 16 bits of a larger size -> the same planes, rounded and area-averaged in the same pass.  Egress: the final pictures (int16, padded) -> 8-bit pictures, and the exact sums of
// squared differences against the int16 source planes of a picture slot; the final pictures or the slots' pictures -> RGB pictures in any of the ingest's forms, colour
// converted in the same pass (yuv_rgb.h), and the exact sums of squared differences against the caller's RGB pictures.  SSIM: the exact window sums between a final picture and a slot (ssim_window.h).  Scene-cut statistics: exact sums between two slots of an encoder (cut_stats.h).
// What the file holds, in its order: the ten job structs (one picture of a launch each; the kernels read a table of them); hmr_picture_launch, which finds kernel and
// grid size by the job type; one builder per job type (descriptors, planes, strides and sizes in, a job out - no encoder); JobRing, the tables of one job type that one
// encoder has in flight, and PictureRings, its ten rings; run_jobs, which queues one launch ordered against the caller's stream by events (k_encode_picture_io.inc and
// the host-memory entries of k_encode_object.inc use it).  The host-only part of the module - builders, descriptor checks, host twins, metrics - is picture_host.cpp.
#pragma once
#include <algorithm>
#include <functional>
#include <tuple>
#include <vector>
#include "common.h"
#include "rgb_yuv.h"
#include "yuv_depth.h"
#include "yuv_rgb.h"
#include "scale_area.h"
#include "ssim_window.h"
#include "cut_stats.h"

#define PICTURE_MAX_JOBS 512         // pictures per launch (the batch calls' limit)
#define PICTURE_RING 4               // job tables of one direction in flight
#define EGRESS_MAX_WIDTH 8192        // a workgroup's partial sum stays inside 32 bits up to this width (picture_io.hip)

// one picture of an ingest launch
struct IngestJob {
	const uint8_t *src[3];       // I420: Y, U, V; NV12: Y, interleaved UV, unused
	int64_t pitch[3];            // bytes from row to row
	int16_t *dst[3];             // the planes at sample (0, 0); 16-byte aligned
	int32_t stride_y, stride_c;  // elements, multiples of 8
	int32_t width, height, format, reserved;
};

// one picture of an egress launch
struct EgressJob {
	const int16_t *rec[3];       // the final picture's planes at sample (0, 0); 16-byte aligned, read-only
	const int16_t *src[3];       // the slot's planes, or all NULL: no sums
	uint8_t *dst[3];             // I420: Y, U, V; NV12: Y, interleaved UV, unused; or all NULL: no picture
	int64_t pitch[3];            // bytes from row to row of dst
	uint64_t *ssd;               // three sums (zeroed in front of the launch), or NULL
	int32_t stride_y, stride_c;  // of rec, elements, multiples of 8
	int32_t src_stride_y, src_stride_c;
	int32_t width, height, format, reserved;
};

// one picture of an RGB ingest launch (k_ingest_rgb): the caller's RGB picture into the int16 planes, colour-converted by rgb_yuv.h's arithmetic
struct RgbIngestJob {
	const uint8_t *src[3];       // HMR_GPU_RGB_PACKED8: src[0] alone; planar: R, G, B
	int64_t pitch[3];            // bytes from row to row
	int16_t *dst[3];             // the planes at sample (0, 0); 16-byte aligned
	int32_t stride_y, stride_c;  // elements, multiples of 8
	int32_t width, height, format, pixel_bytes;
	int32_t offset[3];           // PACKED8: byte of R, G, B inside a pixel
	RgbMatrix m;                 // the nine coefficients and yoff: a launch mixes matrices and ranges
	int32_t reserved[3];
};
static_assert(sizeof(RgbIngestJob) % 8 == 0, "a table of jobs keeps its pointers aligned");

// one picture of a deep / 4:2:2 / 4:4:4 ingest launch (k_ingest_yuv): the caller's Y'CbCr picture into the int16 planes, rounded to 8-bit 4:2:0 by yuv_depth.h's arithmetic
struct YuvIngestJob {
	const uint8_t *src[3];       // PLANAR: Y, U, V; SEMIPLANAR: Y, interleaved pairs, unused; PACKED422: src[0] alone
	int64_t pitch[3];            // bytes from row to row
	int16_t *dst[3];             // the planes at sample (0, 0); 16-byte aligned
	int32_t stride_y, stride_c;  // elements, multiples of 8
	int32_t width, height;
	YuvForm f;                   // layout, taps, container, shifts and offsets: a launch mixes forms
};
static_assert(sizeof(YuvIngestJob) % 8 == 0, "a table of jobs keeps its pointers aligned");

// one picture of an RGB egress launch (k_egress_rgb): int16 planes (a final picture, a picture slot) into the caller's RGB picture by yuv_rgb.h's arithmetic, and / or
// the sums of squared differences between the 8-bit RGB values and the caller's reference RGB picture
struct RgbEgressJob {
	const int16_t *yuv[3];       // the planes at sample (0, 0); 16-byte aligned, read-only
	const uint8_t *src[3];       // the reference picture (src_format < 0: none) - HMR_GPU_RGB_PACKED8: src[0] alone; planar: R, G, B
	int64_t pitch[3];            // bytes from row to row of src
	uint8_t *dst[3];             // the output picture (format < 0: none), planes as src
	int64_t dst_pitch[3];
	uint64_t *ssd;               // three sums (zeroed in front of the launch), or NULL
	int32_t stride_y, stride_c;  // of yuv, elements, multiples of 8
	int32_t width, height;
	int32_t format, pixel_bytes, offset[3];                // of dst
	int32_t src_format, src_pixel_bytes, src_offset[3];    // of src
	YuvMatrix m;                 // the five coefficients and yoff: a launch mixes matrices and ranges
};
static_assert(sizeof(RgbEgressJob) % 8 == 0, "a table of jobs keeps its pointers aligned");

// one picture of a downscaling ingest launch (k_downscale): the caller's src_w x src_h picture, area-averaged by scale_area.h's arithmetic into the dst_w x dst_h planes
struct ScaleJob {
	const uint8_t *src[3];       // I420: Y, U, V; NV12: Y, interleaved UV, unused
	int64_t pitch[3];            // bytes from row to row
	int16_t *dst[3];             // the planes at sample (0, 0); 16-byte aligned
	int32_t stride_y, stride_c;  // elements, multiples of 8
	int32_t src_w, src_h, dst_w, dst_h, format;
	int32_t tile_rows;           // output rows of a tile: as many as the kernel's LDS holds at this job's horizontal ratio (hmr_scale_job)
	ScaleAxis ax, ay;            // the reduced ratios (the same for luma and chroma) with the reciprocals of dx, dy
	uint32_t den, mden;          // sx * sy and its reciprocal (hmr_scale_magic)
};
static_assert(sizeof(ScaleJob) % 8 == 0, "a table of jobs keeps its pointers aligned");

// one picture of a downscaling RGB ingest launch (k_rgb_ladder): the caller's src_w x src_h RGB picture, converted by rgb_yuv.h's arithmetic sample by sample in
// registers and area-averaged by scale_area.h's into the dst_w x dst_h planes (section 12j: the composition of 12f and 12g without the picture in between)
struct RgbScaleJob {
	const uint8_t *src[3];       // HMR_GPU_RGB_PACKED8: src[0] alone; planar: R, G, B
	int64_t pitch[3];            // bytes from row to row
	int16_t *dst[3];             // the planes at sample (0, 0); 16-byte aligned
	int32_t stride_y, stride_c;  // elements, multiples of 8
	int32_t src_w, src_h, dst_w, dst_h;
	int32_t format, pixel_bytes; // of the RGB picture
	int32_t offset[3];           // PACKED8: byte of R, G, B inside a pixel
	int32_t tile_rows;           // output rows of a tile, as ScaleJob's (hmr_rgb_scale_job)
	RgbMatrix m;                 // the nine coefficients and yoff: a launch mixes matrices and ranges
	ScaleAxis ax, ay;            // the reduced ratios (the same for luma and chroma) with the reciprocals of dx, dy
	uint32_t den, mden;          // sx * sy and its reciprocal (hmr_scale_magic)
};
static_assert(sizeof(RgbScaleJob) % 8 == 0, "a table of jobs keeps its pointers aligned");

// one picture of a downscaling deep / 4:2:2 / 4:4:4 ingest launch (k_yuv_ladder): the caller's src_w x src_h Y'CbCr picture, rounded to 8-bit 4:2:0 by yuv_depth.h's arithmetic
// sample by sample in registers and area-averaged by scale_area.h's into the dst_w x dst_h planes (section 12l: the composition of 12k and 12g without the picture in between)
struct YuvScaleJob {
	const uint8_t *src[3];       // PLANAR: Y, U, V; SEMIPLANAR: Y, interleaved pairs, unused; PACKED422: src[0] alone
	int64_t pitch[3];            // bytes from row to row
	int16_t *dst[3];             // the planes at sample (0, 0); 16-byte aligned
	int32_t stride_y, stride_c;  // elements, multiples of 8
	int32_t src_w, src_h, dst_w, dst_h;
	int32_t tile_rows;           // output rows of a tile, as ScaleJob's (hmr_yuv_scale_job)
	int32_t reserved;
	YuvForm f;                   // layout, taps, container, shifts and offsets: a launch mixes forms
	ScaleAxis ax, ay;            // the reduced ratios (the same for luma and chroma) with the reciprocals of dx, dy
	uint32_t den, mden;          // sx * sy and its reciprocal (hmr_scale_magic)
};
static_assert(sizeof(YuvScaleJob) % 8 == 0, "a table of jobs keeps its pointers aligned");

// one picture of an SSIM launch (k_ssim): the sums of ssim_window.h's window values between the int16 planes a and b
struct SsimJob {
	const int16_t *a[3];         // the slot's planes at sample (0, 0); 16-byte aligned, read-only
	const int16_t *b[3];         // the final picture's planes at sample (0, 0); 16-byte aligned, read-only
	int64_t *sum;                // three sums (zeroed in front of the launch)
	int32_t stride_a_y, stride_a_c, stride_b_y, stride_b_c;      // elements, multiples of 8
	int32_t width, height;       // multiples of 8, at least 16
};
static_assert(sizeof(SsimJob) % 8 == 0, "a table of jobs keeps its pointers aligned");

// one picture of a scene-cut launch (k_cut, then k_cut_finish): cut_stats.h's eight values between the int16 planes cur and prev, two slots of one encoder
struct CutJob {
	const int16_t *cur[3];       // the slot just loaded: planes at sample (0, 0); 16-byte aligned, read-only
	const int16_t *prev[3];      // the slot of the frame before
	int64_t *stats;              // HMR_CUT_VALUES values (zeroed in front of the launch)
	uint32_t *bins;              // 2 x 256 counts, the luma histograms of cur and of prev (library-owned: PictureRings::cut_bins; zeroed in front of the launch)
	int32_t stride_y, stride_c;  // elements, multiples of 8 (both slots have the same)
	int32_t width, height;       // multiples of 8
};
static_assert(sizeof(CutJob) % 8 == 0, "a table of jobs keeps its pointers aligned");
static_assert(HMR_CUT_VALUES == HMR_GPU_CUT_VALUES && HMR_CUT_RANGE == HMR_GPU_CUT_RANGE, "cut_stats.h and the public header agree");

// The job table goes from page-locked host memory (`h_jobs`, which must stay untouched until the work queued here has run) to `d_jobs`, then ONE launch of the job
// type's kernel - k_ingest / k_ingest_rgb / k_ingest_yuv / k_downscale / k_rgb_ladder / k_yuv_ladder / k_egress / k_egress_rgb / k_ssim / k_cut (with k_cut_finish behind it) - handles all n pictures; both on `stream`,
// nothing is waited for.  Instantiated in picture_io.hip for the ten job types (PictureKernel there names each type's kernel and grid size).
template <class Job>
int hmr_picture_launch(hipStream_t stream, const Job *h_jobs, Job *d_jobs, int n);

// ---- the job of one picture, one builder per job type (picture_host.cpp; the three scale jobs next to scale_tile in picture_io.hip) ----
// The descriptors have passed their checks.  `dst` and every other int16 plane pointer is the plane at sample (0, 0), with its strides in elements.
// what the six ingest-side jobs begin with: the caller's planes and pitches, the int16 planes and their strides
template <class Job, class Picture>
void hmr_job_planes(Job &j, const Picture &pic, int16_t *const dst[3], int stride_y, int stride_c)
{
	for (int c = 0; c < 3; c++) {
		j.src[c] = (const uint8_t *)pic.plane[c];
		j.pitch[c] = pic.pitch[c];
		j.dst[c] = dst[c];
	}
	j.stride_y = stride_y; j.stride_c = stride_c;
}
// an RGB source (RgbIngestJob, RgbScaleJob): the planes, and how a pixel is read and converted
template <class Job>
void hmr_rgb_source(Job &j, const hmr_gpu_rgb_picture &pic, int16_t *const dst[3], int stride_y, int stride_c)
{
	hmr_job_planes(j, pic, dst, stride_y, stride_c);
	for (int c = 0; c < 3; c++) j.offset[c] = pic.offset[c];
	j.format = pic.format; j.pixel_bytes = pic.pixel_bytes;
	j.m = hmr_rgb_matrix(pic.matrix, pic.full_range);
}
// k_ingest: the 8-bit width x height picture `pic` into the planes `dst`
IngestJob hmr_ingest_job(const hmr_gpu_picture &pic, int16_t *const dst[3], int stride_y, int stride_c, int width, int height);
// k_ingest_rgb, k_ingest_yuv: the same for an RGB picture and for a Y'CbCr picture of any depth and chroma format
RgbIngestJob hmr_rgb_ingest_job(const hmr_gpu_rgb_picture &pic, int16_t *const dst[3], int stride_y, int stride_c, int width, int height);
YuvIngestJob hmr_yuv_ingest_job(const hmr_gpu_yuv_picture &pic, int16_t *const dst[3], int stride_y, int stride_c, int width, int height);
// k_downscale: the sizes have passed hmr_gpu_scale_check; the ratios, their reciprocals and the tile height are derived here
ScaleJob hmr_scale_job(const hmr_gpu_picture &pic, int src_w, int src_h, int16_t *const dst[3], int stride_y, int stride_c, int dst_w, int dst_h);
// k_rgb_ladder: the same for an RGB source, whose descriptor has passed hmr_gpu_rgb_picture_check for the source's size
RgbScaleJob hmr_rgb_scale_job(const hmr_gpu_rgb_picture &pic, int src_w, int src_h, int16_t *const dst[3], int stride_y, int stride_c, int dst_w, int dst_h);
// k_yuv_ladder: the same for a Y'CbCr source of any depth and chroma format, whose descriptor has passed hmr_gpu_yuv_picture_check for the source's size
YuvScaleJob hmr_yuv_scale_job(const hmr_gpu_yuv_picture &pic, int src_w, int src_h, int16_t *const dst[3], int stride_y, int stride_c, int dst_w, int dst_h);
// k_egress: the planes `rec` (a final picture, a picture slot) into `pic` (NULL: no picture), the sums of their squared differences against the planes `src` of a
// picture slot (NULL: none) into ssd
EgressJob hmr_egress_job(int16_t *const rec[3], int stride_y, int stride_c, const hmr_gpu_picture *pic, int16_t *const src[3], int src_stride_y, int src_stride_c, uint64_t *ssd,
			 int width, int height);
// k_egress_rgb: the planes `yuv` into `out` (NULL: no picture), the sums of squared differences against `ref` (NULL: none) into ssd; one of the two is given
RgbEgressJob hmr_rgb_egress_job(int16_t *const yuv[3], int stride_y, int stride_c, const hmr_gpu_rgb_picture *out, const hmr_gpu_rgb_picture *ref, uint64_t *ssd, int width, int height);
// k_ssim: the window sums between the planes a (a picture slot) and b (a final picture) into sum
SsimJob hmr_ssim_job(int16_t *const a[3], int stride_a_y, int stride_a_c, int16_t *const b[3], int stride_b_y, int stride_b_c, int64_t *sum, int width, int height);
// k_cut: cut_stats.h's values of the planes cur against prev (two slots of one encoder: one pair of strides) into stats, the luma histograms through bins
CutJob hmr_cut_job(int16_t *const cur[3], int16_t *const prev[3], int stride_y, int stride_c, int64_t *stats, uint32_t *bins, int width, int height);

// The job tables of the calls one encoder leads, in one direction: a ring of tables in page-locked memory (a table is written again only when the launch that read it
// is known to be over: ev_turn), their copy on the device, the events towards the outside stream (producer or consumer) and towards the streams that go on behind a launch.
template <class Job>
struct JobRing {
	Job *h = nullptr, *d = nullptr;
	int cap = 0, next = 0;
	hipEvent_t ev_turn[PICTURE_RING] = {nullptr, nullptr, nullptr, nullptr}, ev_outside = nullptr, ev_done = nullptr;

	// made at the first call (or a larger one: the work `st` holds, which reads the old tables, is waited for)
	int prepare(int n, hipStream_t st)
	{
		if (!ev_done) {
			for (hipEvent_t &ev : ev_turn) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
			HIP_TRY(hipEventCreateWithFlags(&ev_outside, hipEventDisableTiming));
			HIP_TRY(hipEventCreateWithFlags(&ev_done, hipEventDisableTiming));
		}
		if (n <= cap) return HMR_GPU_OK;
		HIP_TRY(hipStreamSynchronize(st));
		if (h) (void)hipHostFree(h);
		if (d) (void)hipFree(d);
		h = d = nullptr;
		cap = 0;
		const int want = n == 1 ? 1 : PICTURE_MAX_JOBS;
		HIP_TRY(hipHostMalloc((void **)&h, (size_t)PICTURE_RING * want * sizeof(Job), hipHostMallocDefault));
		HIP_TRY(hipMalloc((void **)&d, (size_t)want * sizeof(Job)));
		cap = want;
		next = 0;
		return HMR_GPU_OK;
	}
	// the next table of the ring and the event to record behind the launch that reads it
	int next_table(Job **table, hipEvent_t *turn)
	{
		*turn = ev_turn[next];
		*table = h + (size_t)next * cap;
		next = (next + 1) % PICTURE_RING;
		HIP_TRY(hipEventSynchronize(*turn));      // (the launch of PICTURE_RING calls ago: over long since; an event never recorded counts as complete)
		return HMR_GPU_OK;
	}
	void release()
	{
		if (h) (void)hipHostFree(h);
		if (d) (void)hipFree(d);
		for (hipEvent_t ev : {ev_turn[0], ev_turn[1], ev_turn[2], ev_turn[3], ev_outside, ev_done})
			if (ev) (void)hipEventDestroy(ev);
	}
};

// The rings of one encoder, one per job type (a table is reused after PICTURE_RING calls of ITS kind): a new kernel adds its job type here and nowhere else.
struct PictureRings {
	std::tuple<JobRing<IngestJob>, JobRing<RgbIngestJob>, JobRing<YuvIngestJob>, JobRing<ScaleJob>, JobRing<RgbScaleJob>, JobRing<YuvScaleJob>, JobRing<EgressJob>, JobRing<RgbEgressJob>, JobRing<SsimJob>, JobRing<CutJob>> of;
	uint32_t *cut_bins = nullptr;      // k_cut's histogram bins, 2 x 256 words per picture of a call this encoder leads (hmr_gpu_enc_cut_stats)
	int cut_bins_cap = 0;              // pictures
	void release()
	{
		std::apply([](auto &...ring) { (ring.release(), ...); }, of);
		if (cut_bins) (void)hipFree(cut_bins);
	}
};

// One launch (hmr_picture_launch) over n jobs on `st`, with the ring of the job's type, behind what the `outside` stream holds now and behind whatever `before` queues
// (it may add to `behind`); every distinct stream of `behind` goes on behind the launch.  The host waits for nothing but the ring's turn.
template <class Job>
int run_jobs(PictureRings &rings, hipStream_t st, const Job *jobs, int n, hipStream_t outside, std::vector<hipStream_t> behind = {},
	     const std::function<int(std::vector<hipStream_t> &)> &before = nullptr)
{
	JobRing<Job> &ring = std::get<JobRing<Job>>(rings.of);
	int rc = ring.prepare(n, st);
	if (rc) return rc;
	Job *table;
	hipEvent_t turn;
	if ((rc = ring.next_table(&table, &turn))) return rc;
	std::copy(jobs, jobs + n, table);
	if (outside != st) {
		HIP_TRY(hipEventRecord(ring.ev_outside, outside));
		HIP_TRY(hipStreamWaitEvent(st, ring.ev_outside, 0));
	}
	if (before && (rc = before(behind))) return rc;
	if ((rc = hmr_picture_launch(st, table, ring.d, n))) return rc;
	HIP_TRY(hipEventRecord(turn, st));
	std::sort(behind.begin(), behind.end());
	behind.erase(std::unique(behind.begin(), behind.end()), behind.end());
	behind.erase(std::remove(behind.begin(), behind.end(), st), behind.end());
	if (behind.empty()) return HMR_GPU_OK;
	HIP_TRY(hipEventRecord(ring.ev_done, st));
	for (hipStream_t w : behind) HIP_TRY(hipStreamWaitEvent(w, ring.ev_done, 0));
	return HMR_GPU_OK;
}
