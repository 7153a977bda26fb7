// Host side of the frame encoder, part 3 (included by k_encode.hip): pictures that already lie in device memory, and pictures and quality left there
// (include/homer_gpu.h sections 12d .. 12m).  One call handles the pictures of up to PICTURE_MAX_JOBS encoders with one launch of the job type's kernel (picture_io.hip)
// on the FIRST encoder's stream; run_jobs (picture_io.h) orders it by events and the host waits for nothing.
//   load:   behind the producer's stream; the other encoders' streams and whatever the producer queues next go on behind it.
//   export: behind the consumer's stream (which may still use the output memory), behind the streams that wrote the final pictures and behind the encoders' own
//           streams (which may still load the slots); the consumer's stream and all of those streams go on behind it.
//   ssim:   ordered as export; the final pictures and the slots are read, three sums per encoder are written.
//   cut stats: ordered as export, without the final pictures' writers; two slots are read, eight values per encoder are written.
//   export as RGB: ordered as export; the consumer's stream is also the one that holds the producer of the reference pictures.
// The six load entries are ONE body (load_sources) over a description of their kind of picture; the four export / metric entries share their refusals
// (refuse_encoder), their plane check (check_planes) and their ordering (run_export).  Every job comes from picture_io.h's builders; the host-memory entries of
// k_encode_object.inc (widen_packed, narrow_packed) build theirs for a packed picture - the staging buffer, a picture between GPUs - and run the same kernels.
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
// the planes a descriptor's format has
int planes_of(const hmr_gpu_picture &pic) { return pic.format == HMR_GPU_PIC_NV12 ? 2 : 3; }
int planes_of(const hmr_gpu_rgb_picture &pic) { return pic.format == HMR_GPU_RGB_PACKED8 ? 1 : 3; }
int planes_of(const hmr_gpu_yuv_picture &pic) { return pic.format == HMR_GPU_YUV_PLANAR ? 3 : pic.format == HMR_GPU_YUV_SEMIPLANAR ? 2 : 1; }
// every plane of picture i is device memory of `device`; `prefix` names the array of a call that has two ("outs ", "refs ")
template <class Picture>
int check_planes(const char *fn, int i, const Picture &pic, int device, const char *prefix = "")
{
	for (int c = 0; c < planes_of(pic); c++)
		if (!on_device(pic.plane[c], device)) {
			char what[32];
			snprintf(what, sizeof what, "%splane[%d]", prefix, c);
			return not_device(fn, i, what, device);
		}
	return HMR_GPU_OK;
}
// the three sums of each of n encoders are device memory of `device`
bool sums_on_device(const void *sums, int n, int device) { return on_device(sums, device) && on_device((const uint64_t *)sums + 3 * (size_t)n - 1, device); }
// a refusal of one of the descriptor checks, as the refusal of picture i with `prefix` in front
int refuse_descriptor(const char *fn, int i, const char *prefix = "")
{
	const std::string why = prefix + std::string(hmr_gpu_last_error());
	return picture_refuse(fn, i, why.c_str());
}

// what the load calls of sections 12d, 12f, 12g, 12j, 12k and 12l refuse before they look at a picture
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

// The kinds of picture a load call takes.  Each names its job, checks a descriptor against the encoder's picture size (the scaled kinds: against the SOURCE's size,
// then the pair of sizes), gives the descriptor whose planes have to be device memory, and builds the job of one picture into the planes `dst` of a slot.
struct Load8 {      // section 12d
	typedef IngestJob Job;
	static int check(const hmr_gpu_picture &p, const Seq &s) { return hmr_gpu_picture_check(&p, s.width, s.height); }
	static const hmr_gpu_picture &planes(const hmr_gpu_picture &p) { return p; }
	static Job job(const hmr_gpu_picture &p, int16_t *const dst[3], const Seq &s) { return hmr_ingest_job(p, dst, s.src_stride_y, s.src_stride_c, s.width, s.height); }
};
struct LoadRgb {      // section 12f
	typedef RgbIngestJob Job;
	static int check(const hmr_gpu_rgb_picture &p, const Seq &s) { return hmr_gpu_rgb_picture_check(&p, s.width, s.height); }
	static const hmr_gpu_rgb_picture &planes(const hmr_gpu_rgb_picture &p) { return p; }
	static Job job(const hmr_gpu_rgb_picture &p, int16_t *const dst[3], const Seq &s) { return hmr_rgb_ingest_job(p, dst, s.src_stride_y, s.src_stride_c, s.width, s.height); }
};
struct LoadYuv {      // section 12k
	typedef YuvIngestJob Job;
	static int check(const hmr_gpu_yuv_picture &p, const Seq &s) { return hmr_gpu_yuv_picture_check(&p, s.width, s.height); }
	static const hmr_gpu_yuv_picture &planes(const hmr_gpu_yuv_picture &p) { return p; }
	static Job job(const hmr_gpu_yuv_picture &p, int16_t *const dst[3], const Seq &s) { return hmr_yuv_ingest_job(p, dst, s.src_stride_y, s.src_stride_c, s.width, s.height); }
};
struct LoadScaled {      // section 12g
	typedef ScaleJob Job;
	static int check(const hmr_gpu_scaled_picture &p, const Seq &s)
	{
		const int rc = hmr_gpu_picture_check(&p.pic, p.width, p.height);
		return rc ? rc : hmr_gpu_scale_check(p.width, p.height, s.width, s.height);
	}
	static const hmr_gpu_picture &planes(const hmr_gpu_scaled_picture &p) { return p.pic; }
	static Job job(const hmr_gpu_scaled_picture &p, int16_t *const dst[3], const Seq &s) { return hmr_scale_job(p.pic, p.width, p.height, dst, s.src_stride_y, s.src_stride_c, s.width, s.height); }
};
struct LoadScaledRgb {      // section 12j
	typedef RgbScaleJob Job;
	static int check(const hmr_gpu_scaled_rgb_picture &p, const Seq &s)
	{
		const int rc = hmr_gpu_rgb_picture_check(&p.pic, p.width, p.height);
		return rc ? rc : hmr_gpu_scale_check(p.width, p.height, s.width, s.height);
	}
	static const hmr_gpu_rgb_picture &planes(const hmr_gpu_scaled_rgb_picture &p) { return p.pic; }
	static Job job(const hmr_gpu_scaled_rgb_picture &p, int16_t *const dst[3], const Seq &s) { return hmr_rgb_scale_job(p.pic, p.width, p.height, dst, s.src_stride_y, s.src_stride_c, s.width, s.height); }
};
struct LoadScaledYuv {      // section 12l
	typedef YuvScaleJob Job;
	static int check(const hmr_gpu_scaled_yuv_picture &p, const Seq &s)
	{
		const int rc = hmr_gpu_yuv_picture_check(&p.pic, p.width, p.height);
		return rc ? rc : hmr_gpu_scale_check(p.width, p.height, s.width, s.height);
	}
	static const hmr_gpu_yuv_picture &planes(const hmr_gpu_scaled_yuv_picture &p) { return p.pic; }
	static Job job(const hmr_gpu_scaled_yuv_picture &p, int16_t *const dst[3], const Seq &s) { return hmr_yuv_scale_job(p.pic, p.width, p.height, dst, s.src_stride_y, s.src_stride_c, s.width, s.height); }
};

// A load call of any kind: the refusals in their order, the slots, one job per picture and ONE launch on the first encoder's stream.  The pictures are complete when
// what the producer's stream holds now has run; every other encoder's stream (an encode call starts there: set-up copies, ev_ready) and the producer's (it may write the
// pictures again) go on behind the ingest.
template <class Kind, class Picture>
int load_sources(const char *fn, hmr_gpu_enc **encs, int n, const int *slots, const Picture *pics, void *producer_stream)
{
	int rc;
	if ((rc = check_load(fn, encs, n, slots, pics))) return rc;
	const int device = encs[0]->ctx->device;
	for (int i = 0; i < n; i++)
		if (Kind::check(pics[i], encs[i]->seq) != HMR_GPU_OK) return refuse_descriptor(fn, i);
	HIP_TRY(hipSetDevice(device));
	for (int i = 0; i < n; i++)
		if ((rc = check_planes(fn, i, Kind::planes(pics[i]), device))) return rc;
	if ((rc = make_slots(encs, n, slots))) return rc;
	std::vector<typename Kind::Job> jobs(n);
	for (int i = 0; i < n; i++) jobs[i] = Kind::job(pics[i], encs[i]->src[slots[i]].p, encs[i]->seq);
	hipStream_t producer = (hipStream_t)producer_stream;
	std::vector<hipStream_t> behind(1, producer);
	for (int i = 1; i < n; i++) behind.push_back(encs[i]->ctx->stream);
	return run_jobs(encs[0]->rings, encs[0]->ctx->stream, jobs.data(), n, producer, behind);
}
}  // namespace

extern "C" int hmr_gpu_enc_load_sources_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_picture *pics, void *producer_stream)
{
	return load_sources<Load8>("hmr_gpu_enc_load_sources_device", encs, n, slots, pics, producer_stream);
}
extern "C" int hmr_gpu_enc_load_source_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_picture *pic, void *producer_stream)
{
	return hmr_gpu_enc_load_sources_device(&enc, 1, &slot, pic, producer_stream);
}

// ---- section 12f: RGB pictures in ----
extern "C" int hmr_gpu_enc_load_sources_rgb_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_rgb_picture *pics, void *producer_stream)
{
	return load_sources<LoadRgb>("hmr_gpu_enc_load_sources_rgb_device", encs, n, slots, pics, producer_stream);
}
extern "C" int hmr_gpu_enc_load_source_rgb_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_rgb_picture *pic, void *producer_stream)
{
	return hmr_gpu_enc_load_sources_rgb_device(&enc, 1, &slot, pic, producer_stream);
}

// ---- section 12k: Y'CbCr pictures of 8 .. 16 bits, 4:2:0 / 4:2:2 / 4:4:4, planar, semi-planar or packed, rounded to 8-bit 4:2:0 ----
extern "C" int hmr_gpu_enc_load_sources_yuv_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_yuv_picture *pics, void *producer_stream)
{
	return load_sources<LoadYuv>("hmr_gpu_enc_load_sources_yuv_device", encs, n, slots, pics, producer_stream);
}
extern "C" int hmr_gpu_enc_load_source_yuv_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_yuv_picture *pic, void *producer_stream)
{
	return hmr_gpu_enc_load_sources_yuv_device(&enc, 1, &slot, pic, producer_stream);
}

// ---- section 12g: larger pictures in, area-averaged down to the encoders' sizes ----
extern "C" int hmr_gpu_enc_load_sources_scaled_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_scaled_picture *pics, void *producer_stream)
{
	return load_sources<LoadScaled>("hmr_gpu_enc_load_sources_scaled_device", encs, n, slots, pics, producer_stream);
}
extern "C" int hmr_gpu_enc_load_source_scaled_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_scaled_picture *pic, void *producer_stream)
{
	return hmr_gpu_enc_load_sources_scaled_device(&enc, 1, &slot, pic, producer_stream);
}

// ---- section 12j: larger RGB pictures in, converted and area-averaged down to the encoders' sizes ----
extern "C" int hmr_gpu_enc_load_sources_scaled_rgb_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_scaled_rgb_picture *pics, void *producer_stream)
{
	return load_sources<LoadScaledRgb>("hmr_gpu_enc_load_sources_scaled_rgb_device", encs, n, slots, pics, producer_stream);
}
extern "C" int hmr_gpu_enc_load_source_scaled_rgb_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_scaled_rgb_picture *pic, void *producer_stream)
{
	return hmr_gpu_enc_load_sources_scaled_rgb_device(&enc, 1, &slot, pic, producer_stream);
}

// ---- section 12l: larger Y'CbCr pictures of 8 .. 16 bits in, rounded to 8-bit 4:2:0 and area-averaged down to the encoders' sizes ----
extern "C" int hmr_gpu_enc_load_sources_scaled_yuv(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_scaled_yuv_picture *pics, void *producer_stream)
{
	return load_sources<LoadScaledYuv>("hmr_gpu_enc_load_sources_scaled_yuv", encs, n, slots, pics, producer_stream);
}
extern "C" int hmr_gpu_enc_load_source_scaled_yuv(hmr_gpu_enc *enc, int slot, const hmr_gpu_scaled_yuv_picture *pic, void *producer_stream)
{
	return hmr_gpu_enc_load_sources_scaled_yuv(&enc, 1, &slot, pic, producer_stream);
}

namespace {
// What the export and metric calls refuse of encoder i, tried in this order; a call asks for what it requires and does its own checks in between.
enum { ENCODER = 1, HAS_PICTURE = 2, HAS_SLOT = 4, SUMS_WIDTH = 8 };
int refuse_encoder(const char *fn, hmr_gpu_enc **encs, int i, int what, int slot = -1)
{
	hmr_gpu_enc *e = encs[i];
	if (what & ENCODER) {
		if (!e) return picture_refuse(fn, i, "the encoder is NULL");
		if (e->ctx->device != encs[0]->ctx->device) return picture_refuse(fn, i, "the encoder is on another device than the call's first");
	}
	if ((what & HAS_PICTURE) && !e->has_picture) return picture_refuse(fn, i, "the encoder has not encoded a picture yet");
	if ((what & HAS_SLOT) && (slot < 0 || slot >= (int)e->src.size())) return picture_refuse(fn, i, "the slot does not exist");
	if ((what & SUMS_WIDTH) && e->seq.width > EGRESS_MAX_WIDTH) return picture_refuse(fn, i, "sums are made for pictures up to 8192 samples wide");
	return HMR_GPU_OK;
}

// What a launch on `st` that reads the encoders' final pictures and picture slots has to follow, besides the consumer (its work on the output memory: run_jobs): the
// launches that wrote the final pictures (`final_pictures`; a call that reads the slots alone leaves them out) and what the encoders' own streams hold (loads into the
// slots), every distinct stream once.  The consumer reads the results behind the launch; a later encode call rewrites the final picture, a later load the slot: those
// streams are added to `behind` and go on behind it too.  An encoder that has not encoded anything has no final picture and no stream that wrote one: only its own
// stream counts (the RGB export of a slot, section 12i; the other callers refuse such an encoder before they come here).
int wait_for_writers(hmr_gpu_enc **encs, int n, hipStream_t st, hipStream_t consumer, std::vector<hipStream_t> &behind, bool final_pictures)
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
			if (k == 0 && !(final_pictures && e->has_picture)) continue;      // (a slot's picture alone is asked for, or nothing has written a final picture: section 12i)
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
// ONE launch over the jobs of an export or metric call on the first encoder's stream: behind the consumer (its work on the output memory and on the sums, the producer
// of reference pictures), the writers of the final pictures and the loads into the slots; the sums (three 64-bit words per encoder, or NULL) are zeroed on the launch's
// stream, behind all of them.  The consumer's stream and all of those streams go on behind the launch.
template <class Job>
int run_export(hmr_gpu_enc **encs, int n, const Job *jobs, void *consumer_stream, void *sums, bool final_pictures = true)
{
	hipStream_t st = encs[0]->ctx->stream, consumer = (hipStream_t)consumer_stream;
	auto behind_the_writers = [&](std::vector<hipStream_t> &behind) -> int {
		const int rc = wait_for_writers(encs, n, st, consumer, behind, final_pictures);
		if (rc) return rc;
		if (sums) HIP_TRY(hipMemsetAsync(sums, 0, 3 * (size_t)n * sizeof(uint64_t), st));
		return HMR_GPU_OK;
	};
	return run_jobs(encs[0]->rings, st, jobs, n, consumer, std::vector<hipStream_t>(1, consumer), behind_the_writers);
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
		if ((rc = refuse_encoder(fn, encs, i, ENCODER | HAS_PICTURE | (slots ? HAS_SLOT | SUMS_WIDTH : 0), slots ? slots[i] : -1))) return rc;
		if (pics && hmr_gpu_picture_check(&pics[i], encs[i]->seq.width, encs[i]->seq.height) != HMR_GPU_OK) return refuse_descriptor(fn, i);
	}
	const int device = encs[0]->ctx->device;
	HIP_TRY(hipSetDevice(device));
	for (int i = 0; pics && i < n; i++)
		if ((rc = check_planes(fn, i, pics[i], device))) return rc;
	if (dev_ssd && !sums_on_device(dev_ssd, n, device)) return not_device(fn, 0, "dev_ssd", device);
	std::vector<EgressJob> jobs(n);
	for (int i = 0; i < n; i++) {
		const Seq &s = encs[i]->seq;
		jobs[i] = hmr_egress_job(final_planes(encs[i]).p, s.stride_y, s.stride_c, pics ? &pics[i] : nullptr, slots ? encs[i]->src[slots[i]].p : nullptr, s.src_stride_y, s.src_stride_c,
					 dev_ssd ? dev_ssd + 3 * (size_t)i : nullptr, s.width, s.height);
	}
	return run_export(encs, n, jobs.data(), consumer_stream, dev_ssd);
}

extern "C" int hmr_gpu_enc_export_picture_device(hmr_gpu_enc *enc, const hmr_gpu_picture *pic, int slot, uint64_t *dev_ssd, void *consumer_stream)
{
	return hmr_gpu_enc_export_pictures_device(&enc, 1, pic, slot >= 0 ? &slot : nullptr, dev_ssd, consumer_stream);
}

// ---- section 12f: the slots' pictures out ----
extern "C" int hmr_gpu_enc_export_sources_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_picture *outs, void *consumer_stream)
{
	static const char *const fn = "hmr_gpu_enc_export_sources_device";
	if (!encs || !slots || !outs || n < 1 || n > PICTURE_MAX_JOBS) {
		hmr_set_error("%s: needs 1 .. %d encoders with their slots and output pictures (n = %d)", fn, PICTURE_MAX_JOBS, n);
		return HMR_GPU_ERR_ARG;
	}
	int rc;
	for (int i = 0; i < n; i++) {
		if ((rc = refuse_encoder(fn, encs, i, ENCODER | HAS_SLOT, slots[i]))) return rc;
		if (hmr_gpu_picture_check(&outs[i], encs[i]->seq.width, encs[i]->seq.height) != HMR_GPU_OK) return refuse_descriptor(fn, i);
	}
	const int device = encs[0]->ctx->device;
	HIP_TRY(hipSetDevice(device));
	for (int i = 0; i < n; i++)
		if ((rc = check_planes(fn, i, outs[i], device))) return rc;
	// k_egress with the slot's planes and strides in place of the final picture's, and no sums
	std::vector<EgressJob> jobs(n);
	for (int i = 0; i < n; i++) {
		const Seq &s = encs[i]->seq;
		jobs[i] = hmr_egress_job(encs[i]->src[slots[i]].p, s.src_stride_y, s.src_stride_c, &outs[i], nullptr, s.src_stride_y, s.src_stride_c, nullptr, s.width, s.height);
	}
	// behind the consumer and what the encoders' own streams hold (a load into the slot waits there); the final pictures are not read: their writers do not count
	return run_export(encs, n, jobs.data(), consumer_stream, nullptr, false);
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
	int rc;
	for (int i = 0; i < n; i++) {
		if ((rc = refuse_encoder(fn, encs, i, ENCODER))) return rc;
		if (const char *why = hmr_ssim_refusal(encs[i]->seq.width, encs[i]->seq.height)) return picture_refuse(fn, i, why);
		if ((rc = refuse_encoder(fn, encs, i, HAS_PICTURE | HAS_SLOT, slots[i]))) return rc;
	}
	const int device = encs[0]->ctx->device;
	HIP_TRY(hipSetDevice(device));
	if (!sums_on_device(dev_ssim, n, device)) return not_device(fn, 0, "dev_ssim", device);
	std::vector<SsimJob> jobs(n);
	for (int i = 0; i < n; i++) {
		const Seq &s = encs[i]->seq;
		jobs[i] = hmr_ssim_job(encs[i]->src[slots[i]].p, s.src_stride_y, s.src_stride_c, final_planes(encs[i]).p, s.stride_y, s.stride_c, dev_ssim + 3 * (size_t)i, s.width, s.height);
	}
	return run_export(encs, n, jobs.data(), consumer_stream, dev_ssim);
}

extern "C" int hmr_gpu_enc_ssim_one_device(hmr_gpu_enc *enc, int slot, int64_t *dev_ssim, void *consumer_stream)
{
	return hmr_gpu_enc_ssim_device(&enc, 1, &slot, dev_ssim, consumer_stream);
}

// ---- section 12m: scene-cut statistics between two picture slots ----
extern "C" int hmr_gpu_enc_cut_stats(hmr_gpu_enc **encs, int n, const int *slots, const int *prev_slots, int64_t *dev_stats, void *consumer_stream)
{
	static const char *const fn = "hmr_gpu_enc_cut_stats";
	if (!encs || !slots || !prev_slots || !dev_stats || n < 1 || n > PICTURE_MAX_JOBS) {
		hmr_set_error("%s: needs 1 .. %d encoders with their slots, previous slots and dev_stats (n = %d)", fn, PICTURE_MAX_JOBS, n);
		return HMR_GPU_ERR_ARG;
	}
	int rc;
	for (int i = 0; i < n; i++) {
		if ((rc = refuse_encoder(fn, encs, i, ENCODER | HAS_SLOT, slots[i]))) return rc;
		if (prev_slots[i] < 0 || prev_slots[i] >= (int)encs[i]->src.size()) return picture_refuse(fn, i, "the previous slot does not exist");
		if (slots[i] == prev_slots[i]) return picture_refuse(fn, i, "the slot and the previous slot are the same");
		if (const char *why = hmr_cut_refusal(encs[i]->seq.width, encs[i]->seq.height)) return picture_refuse(fn, i, why);
	}
	const int device = encs[0]->ctx->device;
	HIP_TRY(hipSetDevice(device));
	if (!on_device(dev_stats, device) || !on_device(dev_stats + HMR_CUT_VALUES * (size_t)n - 1, device)) return not_device(fn, 0, "dev_stats", device);
	hipStream_t st = encs[0]->ctx->stream, consumer = (hipStream_t)consumer_stream;
	// the histogram bins of the call's pictures belong to the encoder that leads it (as the job tables do); made at the first call, or a larger one
	PictureRings &rings = encs[0]->rings;
	if (n > rings.cut_bins_cap) {
		HIP_TRY(hipStreamSynchronize(st));      // (a launch that still counts in the old bins)
		if (rings.cut_bins) (void)hipFree(rings.cut_bins);
		rings.cut_bins = nullptr;
		rings.cut_bins_cap = 0;
		const int want = n == 1 ? 1 : PICTURE_MAX_JOBS;
		HIP_TRY(hipMalloc((void **)&rings.cut_bins, (size_t)want * 512 * sizeof(uint32_t)));
		rings.cut_bins_cap = want;
	}
	std::vector<CutJob> jobs(n);
	for (int i = 0; i < n; i++) {
		const Seq &s = encs[i]->seq;
		jobs[i] = hmr_cut_job(encs[i]->src[slots[i]].p, encs[i]->src[prev_slots[i]].p, s.src_stride_y, s.src_stride_c, dev_stats + HMR_CUT_VALUES * (size_t)i, rings.cut_bins + 512 * (size_t)i,
				      s.width, s.height);
	}
	// ordered as 12h's call, but the final pictures are not read: behind the consumer and what the encoders' own streams hold (a load into a slot); the values and the
	// bins are zeroed on the launch's stream behind all of them
	auto behind_the_loads = [&](std::vector<hipStream_t> &behind) -> int {
		const int rc = wait_for_writers(encs, n, st, consumer, behind, false);
		if (rc) return rc;
		HIP_TRY(hipMemsetAsync(dev_stats, 0, HMR_CUT_VALUES * (size_t)n * sizeof(int64_t), st));
		HIP_TRY(hipMemsetAsync(rings.cut_bins, 0, (size_t)n * 512 * sizeof(uint32_t), st));
		return HMR_GPU_OK;
	};
	return run_jobs(rings, st, jobs.data(), n, consumer, std::vector<hipStream_t>(1, consumer), behind_the_loads);
}

extern "C" int hmr_gpu_enc_cut_stats_one(hmr_gpu_enc *enc, int slot, int prev_slot, int64_t *dev_stats, void *consumer_stream)
{
	return hmr_gpu_enc_cut_stats(&enc, 1, &slot, &prev_slot, dev_stats, consumer_stream);
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
	int rc;
	for (int i = 0; i < n; i++) {
		if ((rc = refuse_encoder(fn, encs, i, ENCODER))) return rc;
		hmr_gpu_enc *e = encs[i];
		if (which[i] < -1) return picture_refuse(fn, i, "which: below -1 (-1: the final picture, otherwise a picture slot)");
		if (which[i] >= (int)e->src.size()) return picture_refuse(fn, i, "which: the slot does not exist");
		if (which[i] == -1 && !e->has_picture) return picture_refuse(fn, i, "which: -1 and the encoder has not encoded a picture yet");
		if (refs && (rc = refuse_encoder(fn, encs, i, SUMS_WIDTH))) return rc;
		for (const hmr_gpu_rgb_picture *pics : {outs, refs})
			if (pics && hmr_gpu_rgb_picture_check(&pics[i], e->seq.width, e->seq.height) != HMR_GPU_OK) return refuse_descriptor(fn, i, pics == outs ? "outs: " : "refs: ");
	}
	const int device = encs[0]->ctx->device;
	HIP_TRY(hipSetDevice(device));
	for (const hmr_gpu_rgb_picture *pics : {outs, refs})
		for (int i = 0; pics && i < n; i++)
			if ((rc = check_planes(fn, i, pics[i], device, pics == outs ? "outs " : "refs "))) return rc;
	if (dev_ssd && !sums_on_device(dev_ssd, n, device)) return not_device(fn, 0, "dev_ssd", device);
	std::vector<RgbEgressJob> jobs(n);
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		const Seq &s = e->seq;
		const bool final_picture = which[i] < 0;
		const SrcSlot yuv = final_picture ? final_planes(e) : e->src[which[i]];
		jobs[i] = hmr_rgb_egress_job(yuv.p, final_picture ? s.stride_y : s.src_stride_y, final_picture ? s.stride_c : s.src_stride_c,
					     outs ? &outs[i] : nullptr, refs ? &refs[i] : nullptr, dev_ssd ? dev_ssd + 3 * (size_t)i : nullptr, s.width, s.height);
	}
	// (the final picture's writer is waited for whenever the encoder has one, even where `which` names a slot)
	return run_export(encs, n, jobs.data(), consumer_stream, dev_ssd);
}

extern "C" int hmr_gpu_enc_export_picture_rgb_device(hmr_gpu_enc *enc, int which, const hmr_gpu_rgb_picture *out, const hmr_gpu_rgb_picture *ref, uint64_t *dev_ssd, void *consumer_stream)
{
	return hmr_gpu_enc_export_pictures_rgb_device(&enc, 1, &which, out, ref, dev_ssd, consumer_stream);
}
