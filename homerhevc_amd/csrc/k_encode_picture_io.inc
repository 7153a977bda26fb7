// Host side of the frame encoder, part 3 (included by k_encode.hip): pictures that already lie in device memory, and pictures and quality left there
// (include/homer_gpu.h sections 12d, 12e, 12f, 12g, 12h, 12i, 12j and 12k).  One call handles the pictures of up to PICTURE_MAX_JOBS encoders with one launch of k_ingest / k_ingest_rgb / k_ingest_yuv / k_downscale / k_rgb_ladder / k_egress / k_ssim / k_egress_rgb (picture_io.hip)
// on the FIRST encoder's stream; run_jobs (picture_io.h) orders it by events and the host waits for nothing.
//   load:   behind the producer's stream; the other encoders' streams and whatever the producer queues next go on behind it.
//   export: behind the consumer's stream (which may still use the output memory), behind the streams that wrote the final pictures and behind the encoders' own
//           streams (which may still load the slots); the consumer's stream and all of those streams go on behind it.
//   ssim:   ordered as export; the final pictures and the slots are read, three sums per encoder are written.
//   export as RGB: ordered as export; the consumer's stream is also the one that holds the producer of the reference pictures.
// Each entry checks the caller's arguments and builds the jobs; the host-memory entries of k_encode_object.inc (widen_packed, narrow_packed) build theirs for a
// packed picture - the staging buffer, a picture between GPUs - and run the same kernels.
#include <unordered_set>
namespace {
int picture_refuse(const char *fn, int i, const char *what)
{
	hmr_set_error("%s: picture %d: %s", fn, i, what);
	return HMR_GPU_ERR_ARG;
}
bool on_device(const void *p, int device)
{
	hipPointerAttribute_t attr;
	memset(&attr, 0, sizeof attr);
	if (hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeDevice && attr.device == device) return true;
	(void)hipGetLastError();
	return false;
}
int not_device(const char *fn, int i, const char *what, int device)
{
	hmr_set_error("%s: picture %d: %s is not device memory of device %d", fn, i, what, device);
	return HMR_GPU_ERR_ARG;
}
// a descriptor against the encoder's picture size
int check_descriptor(const char *fn, int i, const hmr_gpu_picture *pic, const hmr_gpu_enc *e)
{
	if (hmr_gpu_picture_check(pic, e->seq.width, e->seq.height) == HMR_GPU_OK) return HMR_GPU_OK;
	const std::string why = hmr_gpu_last_error();
	return picture_refuse(fn, i, why.c_str());
}
// every plane of every picture is device memory of `device`
int check_planes(const char *fn, const hmr_gpu_picture *pics, int n, int device)
{
	static const char *const names[3] = {"plane[0]", "plane[1]", "plane[2]"};
	for (int i = 0; i < n; i++)
		for (int c = 0; c < (pics[i].format == HMR_GPU_PIC_NV12 ? 2 : 3); c++)
			if (!on_device(pics[i].plane[c], device)) return not_device(fn, i, names[c], device);
	return HMR_GPU_OK;
}
}  // namespace

namespace {
// what the load calls of sections 12d, 12f, 12g, 12j and 12k refuse before they look at a picture
int check_load(const char *fn, hmr_gpu_enc **encs, int n, const int *slots, const void *pics)
{
	static_assert(PICTURE_MAX_JOBS == BATCH_MAX, "a load call feeds a batch call, an export call follows one");
	if (!encs || !slots || !pics || n < 1 || n > PICTURE_MAX_JOBS) {
		hmr_set_error("%s: needs 1 .. %d encoders with their slots and pictures (n = %d)", fn, PICTURE_MAX_JOBS, n);
		return HMR_GPU_ERR_ARG;
	}
	for (int i = 0; i < n; i++) {
		if (!encs[i]) return picture_refuse(fn, i, "the encoder is NULL");
		if (slots[i] < 0 || slots[i] > 4096) return picture_refuse(fn, i, "the slot is outside 0 .. 4096");
		if (encs[i]->ctx->device != encs[0]->ctx->device) return picture_refuse(fn, i, "the encoder is on another device than the call's first");
	}
	// the same (encoder, slot) twice: two pictures into one slot in one launch would leave a mix of them
	std::vector<std::pair<hmr_gpu_enc *, int>> seen(n);
	for (int i = 0; i < n; i++) seen[i] = {encs[i], slots[i]};
	std::sort(seen.begin(), seen.end());
	if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) {
		hmr_set_error("%s: the same encoder and slot twice in one call", fn);
		return HMR_GPU_ERR_ARG;
	}
	return HMR_GPU_OK;
}
// the slots of a load call exist
int make_slots(hmr_gpu_enc **encs, int n, const int *slots)
{
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		while ((int)e->src.size() <= slots[i]) {
			SrcSlot sl;
			for (int c = 0; c < 3; c++) DEV_ALLOC(sl.p[c], e->src_elems[c]);
			e->src.push_back(sl);
		}
	}
	return HMR_GPU_OK;
}
// One launch over the jobs of a load call on the first encoder's stream.  The pictures are complete when what the producer's stream holds now has run; every other
// encoder's stream (an encode call starts there: set-up copies, ev_ready) and the producer's (it may write the pictures again) go on behind the ingest.
template <class Job>
int run_load(JobRing<Job> &ring, int (*launch)(hipStream_t, const Job *, Job *, int), hmr_gpu_enc **encs, int n, const Job *jobs, void *producer_stream)
{
	hipStream_t producer = (hipStream_t)producer_stream;
	std::vector<hipStream_t> behind(1, producer);
	for (int i = 1; i < n; i++) behind.push_back(encs[i]->ctx->stream);
	return run_jobs(ring, launch, encs[0]->ctx->stream, jobs, n, producer, behind);
}
}  // namespace

extern "C" int hmr_gpu_enc_load_sources_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_picture *pics, void *producer_stream)
{
	static const char *const fn = "hmr_gpu_enc_load_sources_device";
	int rc;
	if ((rc = check_load(fn, encs, n, slots, pics))) return rc;
	const int device = encs[0]->ctx->device;
	for (int i = 0; i < n; i++)
		if ((rc = check_descriptor(fn, i, &pics[i], encs[i]))) return rc;
	HIP_TRY(hipSetDevice(device));
	if ((rc = check_planes(fn, pics, n, device))) return rc;
	if ((rc = make_slots(encs, n, slots))) return rc;
	std::vector<IngestJob> jobs(n);
	for (int i = 0; i < n; i++) jobs[i] = ingest_job(encs[i], pics[i], encs[i]->src[slots[i]].p, encs[i]->seq.src_stride_y, encs[i]->seq.src_stride_c);
	return run_load(encs[0]->ingest, hmr_ingest_launch, encs, n, jobs.data(), producer_stream);
}

extern "C" int hmr_gpu_enc_load_source_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_picture *pic, void *producer_stream)
{
	return hmr_gpu_enc_load_sources_device(&enc, 1, &slot, pic, producer_stream);
}

namespace {
// What a launch on `st` that reads the encoders' final pictures and picture slots has to follow, besides the consumer (its work on the output memory: run_jobs): the
// launches that wrote the final pictures and what the encoders' own streams hold (loads into the slots), every distinct stream once.  The consumer reads the results
// behind the launch; a later encode call rewrites the final picture, a later load the slot: those streams are added to `behind` and go on behind it too.
// An encoder that has not encoded anything has no final picture and no stream that wrote one: only its own stream counts (the RGB export of a slot, section 12i; the
// other callers refuse such an encoder before they come here).
int wait_for_writers(hmr_gpu_enc **encs, int n, hipStream_t st, hipStream_t consumer, std::vector<hipStream_t> &behind)
{
	std::unordered_set<hipStream_t> seen = {consumer, st};
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		if (!e->ev_pic_done) {
			HIP_TRY(hipEventCreateWithFlags(&e->ev_pic_done, hipEventDisableTiming));
			HIP_TRY(hipEventCreateWithFlags(&e->ev_own_done, hipEventDisableTiming));
		}
		const hipStream_t wrote[2] = {e->pic_stream, e->ctx->stream};
		hipEvent_t const ev[2] = {e->ev_pic_done, e->ev_own_done};
		for (int k = 0; k < 2; k++) {
			if (k == 0 && !e->has_picture) continue;      // (a slot's picture alone is asked for, section 12i: nothing has written a final picture)
			if (!seen.insert(wrote[k]).second) continue;
			behind.push_back(wrote[k]);
			// a stream with nothing in flight has nothing to queue behind (calls on one encoder come from one host thread at a time: nobody is adding to it now);
			// the query is far cheaper than an event and a wait, and after an encode call most of a batch's streams are idle
			if (hipStreamQuery(wrote[k]) == hipSuccess) continue;
			(void)hipGetLastError();
			HIP_TRY(hipEventRecord(ev[k], wrote[k]));
			HIP_TRY(hipStreamWaitEvent(st, ev[k], 0));
		}
	}
	return HMR_GPU_OK;
}
}  // namespace

extern "C" int hmr_gpu_enc_export_pictures_device(hmr_gpu_enc **encs, int n, const hmr_gpu_picture *pics, const int *slots, uint64_t *dev_ssd, void *consumer_stream)
{
	static const char *const fn = "hmr_gpu_enc_export_pictures_device";
	if (!encs || n < 1 || n > PICTURE_MAX_JOBS) {
		hmr_set_error("%s: needs 1 .. %d encoders (n = %d)", fn, PICTURE_MAX_JOBS, n);
		return HMR_GPU_ERR_ARG;
	}
	if (!pics && !slots) {
		hmr_set_error("%s: neither pictures nor slots: nothing to do", fn);
		return HMR_GPU_ERR_ARG;
	}
	if (!slots != !dev_ssd) {
		hmr_set_error("%s: slots and dev_ssd go together (the sums of squared differences against the slots' pictures)", fn);
		return HMR_GPU_ERR_ARG;
	}
	int rc;
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		if (!e) return picture_refuse(fn, i, "the encoder is NULL");
		if (e->ctx->device != encs[0]->ctx->device) return picture_refuse(fn, i, "the encoder is on another device than the call's first");
		if (!e->has_picture) return picture_refuse(fn, i, "the encoder has not encoded a picture yet");
		if (slots && (slots[i] < 0 || slots[i] >= (int)e->src.size())) return picture_refuse(fn, i, "the slot does not exist");
		if (slots && e->seq.width > EGRESS_MAX_WIDTH) return picture_refuse(fn, i, "sums are made for pictures up to 8192 samples wide");
		if (pics && (rc = check_descriptor(fn, i, &pics[i], e))) return rc;
	}
	const int device = encs[0]->ctx->device;
	HIP_TRY(hipSetDevice(device));
	if (pics && (rc = check_planes(fn, pics, n, device))) return rc;
	if (dev_ssd && (!on_device(dev_ssd, device) || !on_device(dev_ssd + 3 * (size_t)n - 1, device))) return not_device(fn, 0, "dev_ssd", device);
	std::vector<EgressJob> jobs(n);
	for (int i = 0; i < n; i++)
		jobs[i] = egress_job(encs[i], pics ? &pics[i] : nullptr, slots ? encs[i]->src[slots[i]].p : nullptr, dev_ssd ? dev_ssd + 3 * (size_t)i : nullptr);
	hipStream_t st = encs[0]->ctx->stream, consumer = (hipStream_t)consumer_stream;
	auto behind_the_writers = [&](std::vector<hipStream_t> &behind) -> int {
		const int rc = wait_for_writers(encs, n, st, consumer, behind);
		if (rc) return rc;
		if (dev_ssd) HIP_TRY(hipMemsetAsync(dev_ssd, 0, 3 * (size_t)n * sizeof(uint64_t), st));
		return HMR_GPU_OK;
	};
	return run_jobs(encs[0]->egress, hmr_egress_launch, st, jobs.data(), n, consumer, std::vector<hipStream_t>(1, consumer), behind_the_writers);
}

extern "C" int hmr_gpu_enc_export_picture_device(hmr_gpu_enc *enc, const hmr_gpu_picture *pic, int slot, uint64_t *dev_ssd, void *consumer_stream)
{
	return hmr_gpu_enc_export_pictures_device(&enc, 1, pic, slot >= 0 ? &slot : nullptr, dev_ssd, consumer_stream);
}

// ---- section 12f: RGB pictures in, the slots' pictures out ----
extern "C" int hmr_gpu_enc_load_sources_rgb_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_rgb_picture *pics, void *producer_stream)
{
	static const char *const fn = "hmr_gpu_enc_load_sources_rgb_device";
	int rc;
	if ((rc = check_load(fn, encs, n, slots, pics))) return rc;
	const int device = encs[0]->ctx->device;
	for (int i = 0; i < n; i++)
		if (hmr_gpu_rgb_picture_check(&pics[i], encs[i]->seq.width, encs[i]->seq.height) != HMR_GPU_OK) {
			const std::string why = hmr_gpu_last_error();
			return picture_refuse(fn, i, why.c_str());
		}
	HIP_TRY(hipSetDevice(device));
	static const char *const names[3] = {"plane[0]", "plane[1]", "plane[2]"};
	for (int i = 0; i < n; i++)
		for (int c = 0; c < (pics[i].format == HMR_GPU_RGB_PACKED8 ? 1 : 3); c++)
			if (!on_device(pics[i].plane[c], device)) return not_device(fn, i, names[c], device);
	if ((rc = make_slots(encs, n, slots))) return rc;
	std::vector<RgbIngestJob> jobs(n);
	for (int i = 0; i < n; i++) {
		const hmr_gpu_enc *e = encs[i];
		const hmr_gpu_rgb_picture &pic = pics[i];
		RgbIngestJob &j = jobs[i];
		memset(&j, 0, sizeof j);
		for (int c = 0; c < 3; c++) {
			j.src[c] = (const uint8_t *)pic.plane[c];
			j.pitch[c] = pic.pitch[c];
			j.dst[c] = e->src[slots[i]].p[c];
			j.offset[c] = pic.offset[c];
		}
		j.stride_y = e->seq.src_stride_y; j.stride_c = e->seq.src_stride_c;
		j.width = e->seq.width; j.height = e->seq.height;
		j.format = pic.format; j.pixel_bytes = pic.pixel_bytes;
		j.m = hmr_rgb_matrix(pic.matrix, pic.full_range);
	}
	return run_load(encs[0]->ingest_rgb, hmr_ingest_rgb_launch, encs, n, jobs.data(), producer_stream);
}

extern "C" int hmr_gpu_enc_load_source_rgb_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_rgb_picture *pic, void *producer_stream)
{
	return hmr_gpu_enc_load_sources_rgb_device(&enc, 1, &slot, pic, producer_stream);
}

// ---- section 12k: Y'CbCr pictures of 8 .. 16 bits, 4:2:0 / 4:2:2 / 4:4:4, planar, semi-planar or packed, rounded to 8-bit 4:2:0 ----
extern "C" int hmr_gpu_enc_load_sources_yuv_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_yuv_picture *pics, void *producer_stream)
{
	static const char *const fn = "hmr_gpu_enc_load_sources_yuv_device";
	int rc;
	if ((rc = check_load(fn, encs, n, slots, pics))) return rc;
	const int device = encs[0]->ctx->device;
	for (int i = 0; i < n; i++)
		if (hmr_gpu_yuv_picture_check(&pics[i], encs[i]->seq.width, encs[i]->seq.height) != HMR_GPU_OK) {
			const std::string why = hmr_gpu_last_error();
			return picture_refuse(fn, i, why.c_str());
		}
	HIP_TRY(hipSetDevice(device));
	static const char *const names[3] = {"plane[0]", "plane[1]", "plane[2]"};
	for (int i = 0; i < n; i++)
		for (int c = 0; c < (pics[i].format == HMR_GPU_YUV_PLANAR ? 3 : pics[i].format == HMR_GPU_YUV_SEMIPLANAR ? 2 : 1); c++)
			if (!on_device(pics[i].plane[c], device)) return not_device(fn, i, names[c], device);
	if ((rc = make_slots(encs, n, slots))) return rc;
	std::vector<YuvIngestJob> jobs(n);
	for (int i = 0; i < n; i++) {
		const hmr_gpu_enc *e = encs[i];
		const hmr_gpu_yuv_picture &pic = pics[i];
		YuvIngestJob &j = jobs[i];
		memset(&j, 0, sizeof j);
		for (int c = 0; c < 3; c++) {
			j.src[c] = (const uint8_t *)pic.plane[c];
			j.pitch[c] = pic.pitch[c];
			j.dst[c] = e->src[slots[i]].p[c];
		}
		j.stride_y = e->seq.src_stride_y; j.stride_c = e->seq.src_stride_c;
		j.width = e->seq.width; j.height = e->seq.height;
		j.f = hmr_yuv_form(pic.format, pic.chroma, pic.bits, pic.msb_aligned, pic.offset);
	}
	return run_load(encs[0]->ingest_yuv, hmr_ingest_yuv_launch, encs, n, jobs.data(), producer_stream);
}

extern "C" int hmr_gpu_enc_load_source_yuv_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_yuv_picture *pic, void *producer_stream)
{
	return hmr_gpu_enc_load_sources_yuv_device(&enc, 1, &slot, pic, producer_stream);
}

// ---- section 12g: larger pictures in, area-averaged down to the encoders' sizes ----
extern "C" int hmr_gpu_enc_load_sources_scaled_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_scaled_picture *pics, void *producer_stream)
{
	static const char *const fn = "hmr_gpu_enc_load_sources_scaled_device";
	int rc;
	if ((rc = check_load(fn, encs, n, slots, pics))) return rc;
	const int device = encs[0]->ctx->device;
	for (int i = 0; i < n; i++)      // the descriptor against the SOURCE's size, then the pair of sizes
		if (hmr_gpu_picture_check(&pics[i].pic, pics[i].width, pics[i].height) != HMR_GPU_OK ||
		    hmr_gpu_scale_check(pics[i].width, pics[i].height, encs[i]->seq.width, encs[i]->seq.height) != HMR_GPU_OK) {
			const std::string why = hmr_gpu_last_error();
			return picture_refuse(fn, i, why.c_str());
		}
	HIP_TRY(hipSetDevice(device));
	static const char *const names[3] = {"plane[0]", "plane[1]", "plane[2]"};
	for (int i = 0; i < n; i++)
		for (int c = 0; c < (pics[i].pic.format == HMR_GPU_PIC_NV12 ? 2 : 3); c++)
			if (!on_device(pics[i].pic.plane[c], device)) return not_device(fn, i, names[c], device);
	if ((rc = make_slots(encs, n, slots))) return rc;
	std::vector<ScaleJob> jobs(n);
	for (int i = 0; i < n; i++) {
		const hmr_gpu_enc *e = encs[i];
		jobs[i] = hmr_scale_job(pics[i].pic, pics[i].width, pics[i].height, e->src[slots[i]].p, e->seq.src_stride_y, e->seq.src_stride_c, e->seq.width, e->seq.height);
	}
	return run_load(encs[0]->scale, hmr_scale_launch, encs, n, jobs.data(), producer_stream);
}

extern "C" int hmr_gpu_enc_load_source_scaled_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_scaled_picture *pic, void *producer_stream)
{
	return hmr_gpu_enc_load_sources_scaled_device(&enc, 1, &slot, pic, producer_stream);
}

// ---- section 12j: larger RGB pictures in, converted and area-averaged down to the encoders' sizes ----
extern "C" int hmr_gpu_enc_load_sources_scaled_rgb_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_scaled_rgb_picture *pics, void *producer_stream)
{
	static const char *const fn = "hmr_gpu_enc_load_sources_scaled_rgb_device";
	int rc;
	if ((rc = check_load(fn, encs, n, slots, pics))) return rc;
	const int device = encs[0]->ctx->device;
	for (int i = 0; i < n; i++)      // the descriptor against the SOURCE's size, then the pair of sizes
		if (hmr_gpu_rgb_picture_check(&pics[i].pic, pics[i].width, pics[i].height) != HMR_GPU_OK ||
		    hmr_gpu_scale_check(pics[i].width, pics[i].height, encs[i]->seq.width, encs[i]->seq.height) != HMR_GPU_OK) {
			const std::string why = hmr_gpu_last_error();
			return picture_refuse(fn, i, why.c_str());
		}
	HIP_TRY(hipSetDevice(device));
	static const char *const names[3] = {"plane[0]", "plane[1]", "plane[2]"};
	for (int i = 0; i < n; i++)
		for (int c = 0; c < (pics[i].pic.format == HMR_GPU_RGB_PACKED8 ? 1 : 3); c++)
			if (!on_device(pics[i].pic.plane[c], device)) return not_device(fn, i, names[c], device);
	if ((rc = make_slots(encs, n, slots))) return rc;
	std::vector<RgbScaleJob> jobs(n);
	for (int i = 0; i < n; i++) {
		const hmr_gpu_enc *e = encs[i];
		jobs[i] = hmr_rgb_scale_job(pics[i].pic, pics[i].width, pics[i].height, e->src[slots[i]].p, e->seq.src_stride_y, e->seq.src_stride_c, e->seq.width, e->seq.height);
	}
	return run_load(encs[0]->scale_rgb, hmr_rgb_scale_launch, encs, n, jobs.data(), producer_stream);
}

extern "C" int hmr_gpu_enc_load_source_scaled_rgb_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_scaled_rgb_picture *pic, void *producer_stream)
{
	return hmr_gpu_enc_load_sources_scaled_rgb_device(&enc, 1, &slot, pic, producer_stream);
}

extern "C" int hmr_gpu_enc_export_sources_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_picture *outs, void *consumer_stream)
{
	static const char *const fn = "hmr_gpu_enc_export_sources_device";
	if (!encs || !slots || !outs || n < 1 || n > PICTURE_MAX_JOBS) {
		hmr_set_error("%s: needs 1 .. %d encoders with their slots and output pictures (n = %d)", fn, PICTURE_MAX_JOBS, n);
		return HMR_GPU_ERR_ARG;
	}
	int rc;
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		if (!e) return picture_refuse(fn, i, "the encoder is NULL");
		if (e->ctx->device != encs[0]->ctx->device) return picture_refuse(fn, i, "the encoder is on another device than the call's first");
		if (slots[i] < 0 || slots[i] >= (int)e->src.size()) return picture_refuse(fn, i, "the slot does not exist");
		if ((rc = check_descriptor(fn, i, &outs[i], e))) return rc;
	}
	const int device = encs[0]->ctx->device;
	HIP_TRY(hipSetDevice(device));
	if ((rc = check_planes(fn, outs, n, device))) return rc;
	// k_egress with the slot's planes and strides in place of the final picture's, and no sums
	std::vector<EgressJob> jobs(n);
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		EgressJob &j = jobs[i];
		j = egress_job(e, &outs[i], nullptr, nullptr);
		for (int c = 0; c < 3; c++) j.rec[c] = e->src[slots[i]].p[c];
		j.stride_y = e->seq.src_stride_y; j.stride_c = e->seq.src_stride_c;
	}
	hipStream_t st = encs[0]->ctx->stream, consumer = (hipStream_t)consumer_stream;
	// behind the consumer (its work on the output memory: run_jobs) and behind what the encoders' own streams hold (a load into the slot waits there); the consumer
	// reads the output behind the egress, a later load rewrites the slot: those streams go on behind it
	auto behind_the_loads = [&](std::vector<hipStream_t> &behind) -> int {
		std::unordered_set<hipStream_t> seen = {consumer, st};
		for (int i = 0; i < n; i++) {
			hmr_gpu_enc *e = encs[i];
			if (!seen.insert(e->ctx->stream).second) continue;
			behind.push_back(e->ctx->stream);
			if (hipStreamQuery(e->ctx->stream) == hipSuccess) continue;      // (nothing in flight: nothing to queue behind, as in the export of the final pictures)
			(void)hipGetLastError();
			if (!e->ev_pic_done) {
				HIP_TRY(hipEventCreateWithFlags(&e->ev_pic_done, hipEventDisableTiming));
				HIP_TRY(hipEventCreateWithFlags(&e->ev_own_done, hipEventDisableTiming));
			}
			HIP_TRY(hipEventRecord(e->ev_own_done, e->ctx->stream));
			HIP_TRY(hipStreamWaitEvent(st, e->ev_own_done, 0));
		}
		return HMR_GPU_OK;
	};
	return run_jobs(encs[0]->egress, hmr_egress_launch, st, jobs.data(), n, consumer, std::vector<hipStream_t>(1, consumer), behind_the_loads);
}

extern "C" int hmr_gpu_enc_export_source_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_picture *out, void *consumer_stream)
{
	return hmr_gpu_enc_export_sources_device(&enc, 1, &slot, out, consumer_stream);
}

// ---- section 12h: SSIM of the final pictures against picture slots ----
extern "C" int hmr_gpu_enc_ssim_device(hmr_gpu_enc **encs, int n, const int *slots, int64_t *dev_ssim, void *consumer_stream)
{
	static const char *const fn = "hmr_gpu_enc_ssim_device";
	if (!encs || !slots || !dev_ssim || n < 1 || n > PICTURE_MAX_JOBS) {
		hmr_set_error("%s: needs 1 .. %d encoders with their slots and dev_ssim (n = %d)", fn, PICTURE_MAX_JOBS, n);
		return HMR_GPU_ERR_ARG;
	}
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		if (!e) return picture_refuse(fn, i, "the encoder is NULL");
		if (e->ctx->device != encs[0]->ctx->device) return picture_refuse(fn, i, "the encoder is on another device than the call's first");
		if (const char *why = hmr_ssim_refusal(e->seq.width, e->seq.height)) return picture_refuse(fn, i, why);
		if (!e->has_picture) return picture_refuse(fn, i, "the encoder has not encoded a picture yet");
		if (slots[i] < 0 || slots[i] >= (int)e->src.size()) return picture_refuse(fn, i, "the slot does not exist");
	}
	const int device = encs[0]->ctx->device;
	HIP_TRY(hipSetDevice(device));
	if (!on_device(dev_ssim, device) || !on_device(dev_ssim + 3 * (size_t)n - 1, device)) return not_device(fn, 0, "dev_ssim", device);
	std::vector<SsimJob> jobs(n);
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		const Seq &s = e->seq;
		SsimJob &j = jobs[i];
		for (int c = 0; c < 3; c++) {
			j.a[c] = e->src[slots[i]].p[c];
			j.b[c] = plane0(e, e->cur, c);
		}
		j.sum = dev_ssim + 3 * (size_t)i;
		j.stride_a_y = s.src_stride_y; j.stride_a_c = s.src_stride_c;
		j.stride_b_y = s.stride_y; j.stride_b_c = s.stride_c;
		j.width = s.width; j.height = s.height;
	}
	hipStream_t st = encs[0]->ctx->stream, consumer = (hipStream_t)consumer_stream;
	// ordered as the export of 12e: behind the consumer (its work on dev_ssim), the writers of the final pictures and the loads into the slots; the sums are zeroed on
	// the launch's stream, behind all of them
	auto behind_the_writers = [&](std::vector<hipStream_t> &behind) -> int {
		const int rc = wait_for_writers(encs, n, st, consumer, behind);
		if (rc) return rc;
		HIP_TRY(hipMemsetAsync(dev_ssim, 0, 3 * (size_t)n * sizeof(int64_t), st));
		return HMR_GPU_OK;
	};
	return run_jobs(encs[0]->ssim, hmr_ssim_launch, st, jobs.data(), n, consumer, std::vector<hipStream_t>(1, consumer), behind_the_writers);
}

extern "C" int hmr_gpu_enc_ssim_one_device(hmr_gpu_enc *enc, int slot, int64_t *dev_ssim, void *consumer_stream)
{
	return hmr_gpu_enc_ssim_device(&enc, 1, &slot, dev_ssim, consumer_stream);
}

// ---- section 12i: the final pictures or the slots' pictures out as RGB, and their distance to the caller's RGB pictures ----
extern "C" int hmr_gpu_enc_export_pictures_rgb_device(hmr_gpu_enc **encs, int n, const int *which, const hmr_gpu_rgb_picture *outs, const hmr_gpu_rgb_picture *refs, uint64_t *dev_ssd,
						      void *consumer_stream)
{
	static const char *const fn = "hmr_gpu_enc_export_pictures_rgb_device";
	if (!encs || !which || n < 1 || n > PICTURE_MAX_JOBS) {
		hmr_set_error("%s: needs 1 .. %d encoders with `which` (n = %d)", fn, PICTURE_MAX_JOBS, n);
		return HMR_GPU_ERR_ARG;
	}
	if (!outs && !refs) {
		hmr_set_error("%s: neither outs nor refs: nothing to do", fn);
		return HMR_GPU_ERR_ARG;
	}
	if (!refs != !dev_ssd) {
		hmr_set_error("%s: refs and dev_ssd go together (the sums of squared differences against the reference pictures)", fn);
		return HMR_GPU_ERR_ARG;
	}
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		if (!e) return picture_refuse(fn, i, "the encoder is NULL");
		if (e->ctx->device != encs[0]->ctx->device) return picture_refuse(fn, i, "the encoder is on another device than the call's first");
		if (which[i] < -1) return picture_refuse(fn, i, "which: below -1 (-1: the final picture, otherwise a picture slot)");
		if (which[i] >= (int)e->src.size()) return picture_refuse(fn, i, "which: the slot does not exist");
		if (which[i] == -1 && !e->has_picture) return picture_refuse(fn, i, "which: -1 and the encoder has not encoded a picture yet");
		if (refs && e->seq.width > EGRESS_MAX_WIDTH) return picture_refuse(fn, i, "sums are made for pictures up to 8192 samples wide");
		for (const hmr_gpu_rgb_picture *pics : {outs, refs})
			if (pics && hmr_gpu_rgb_picture_check(&pics[i], e->seq.width, e->seq.height) != HMR_GPU_OK) {
				const std::string why = std::string(pics == outs ? "outs: " : "refs: ") + hmr_gpu_last_error();
				return picture_refuse(fn, i, why.c_str());
			}
	}
	const int device = encs[0]->ctx->device;
	HIP_TRY(hipSetDevice(device));
	static const char *const out_names[3] = {"outs plane[0]", "outs plane[1]", "outs plane[2]"}, *const ref_names[3] = {"refs plane[0]", "refs plane[1]", "refs plane[2]"};
	for (const hmr_gpu_rgb_picture *pics : {outs, refs})
		for (int i = 0; pics && i < n; i++)
			for (int c = 0; c < (pics[i].format == HMR_GPU_RGB_PACKED8 ? 1 : 3); c++)
				if (!on_device(pics[i].plane[c], device)) return not_device(fn, i, (pics == outs ? out_names : ref_names)[c], device);
	if (dev_ssd && (!on_device(dev_ssd, device) || !on_device(dev_ssd + 3 * (size_t)n - 1, device))) return not_device(fn, 0, "dev_ssd", device);
	std::vector<RgbEgressJob> jobs(n);
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		const Seq &s = e->seq;
		RgbEgressJob &j = jobs[i];
		memset(&j, 0, sizeof j);
		const bool final_picture = which[i] < 0;
		for (int c = 0; c < 3; c++) {
			j.yuv[c] = final_picture ? plane0(e, e->cur, c) : e->src[which[i]].p[c];
			if (outs) {
				j.dst[c] = (uint8_t *)const_cast<void *>(outs[i].plane[c]);      // (as the output descriptor of 12e: the call writes through the plane pointers)
				j.dst_pitch[c] = outs[i].pitch[c];
				j.offset[c] = outs[i].offset[c];
			}
			if (refs) {
				j.src[c] = (const uint8_t *)refs[i].plane[c];
				j.pitch[c] = refs[i].pitch[c];
				j.src_offset[c] = refs[i].offset[c];
			}
		}
		j.ssd = dev_ssd ? dev_ssd + 3 * (size_t)i : nullptr;
		j.stride_y = final_picture ? s.stride_y : s.src_stride_y; j.stride_c = final_picture ? s.stride_c : s.src_stride_c;
		j.width = s.width; j.height = s.height;
		j.format = outs ? outs[i].format : -1; j.pixel_bytes = outs ? outs[i].pixel_bytes : 0;
		j.src_format = refs ? refs[i].format : -1; j.src_pixel_bytes = refs ? refs[i].pixel_bytes : 0;
		const hmr_gpu_rgb_picture &colour = outs ? outs[i] : refs[i];      // (sums alone: the table comes from the reference's fields)
		j.m = hmr_yuv_matrix(colour.matrix, colour.full_range);
	}
	hipStream_t st = encs[0]->ctx->stream, consumer = (hipStream_t)consumer_stream;
	// ordered as the export of 12e: behind the consumer (its work on the output memory and on dev_ssd, the producer of the reference pictures), the writers of the final
	// pictures and the loads into the slots; the sums are zeroed on the launch's stream, behind all of them
	auto behind_the_writers = [&](std::vector<hipStream_t> &behind) -> int {
		const int rc = wait_for_writers(encs, n, st, consumer, behind);
		if (rc) return rc;
		if (dev_ssd) HIP_TRY(hipMemsetAsync(dev_ssd, 0, 3 * (size_t)n * sizeof(uint64_t), st));
		return HMR_GPU_OK;
	};
	return run_jobs(encs[0]->egress_rgb, hmr_egress_rgb_launch, st, jobs.data(), n, consumer, std::vector<hipStream_t>(1, consumer), behind_the_writers);
}

extern "C" int hmr_gpu_enc_export_picture_rgb_device(hmr_gpu_enc *enc, int which, const hmr_gpu_rgb_picture *out, const hmr_gpu_rgb_picture *ref, uint64_t *dev_ssd, void *consumer_stream)
{
	return hmr_gpu_enc_export_pictures_rgb_device(&enc, 1, &which, out, ref, dev_ssd, consumer_stream);
}
