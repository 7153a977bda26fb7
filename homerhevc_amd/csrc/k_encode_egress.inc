// Host side of the frame encoder, part 4 (included by k_encode.hip): the encoders' final pictures and their distance to a picture slot, left in device memory
// (include/homer_gpu.h section 12e).  One call handles the pictures of up to EGRESS_MAX_JOBS encoders with one launch of k_egress (k_egress.hip) on the FIRST encoder's
// stream.  Events order it behind the consumer's stream (which may still use the output memory), behind the streams that wrote the final pictures and behind the encoders'
// own streams (which may still load the slots); the consumer's stream and all of those streams go on behind it.  The host waits for nothing.
#include <unordered_set>
namespace {
int egress_refuse(const char *fn, int i, const char *what)
{
	hmr_set_error("%s: picture %d: %s", fn, i, what);
	return HMR_GPU_ERR_ARG;
}
int egress_not_device(const char *fn, int i, const char *what, int device)
{
	hmr_set_error("%s: picture %d: %s is not device memory of device %d", fn, i, what, device);
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
// the lead's job tables and events, made when it first leads a call (or a larger one: the work queued with the old tables is waited for)
int egress_prepare(hmr_gpu_enc *lead, int n)
{
	if (!lead->ev_consumer) {
		HIP_TRY(hipEventCreateWithFlags(&lead->ev_consumer, hipEventDisableTiming));
		HIP_TRY(hipEventCreateWithFlags(&lead->ev_egressed, hipEventDisableTiming));
		for (hipEvent_t &ev : lead->ev_ejobs) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
	}
	if (n <= lead->ejobs_cap) return HMR_GPU_OK;
	HIP_TRY(hipStreamSynchronize(lead->ctx->stream));
	if (lead->h_ejobs) (void)hipHostFree(lead->h_ejobs);
	if (lead->d_ejobs) (void)hipFree(lead->d_ejobs);
	lead->h_ejobs = lead->d_ejobs = nullptr;
	lead->ejobs_cap = 0;
	const int cap = n == 1 ? 1 : EGRESS_MAX_JOBS;
	HIP_TRY(hipHostMalloc((void **)&lead->h_ejobs, (size_t)INGEST_RING * cap * sizeof(EgressJob), hipHostMallocDefault));
	HIP_TRY(hipMalloc((void **)&lead->d_ejobs, (size_t)cap * sizeof(EgressJob)));
	lead->ejobs_cap = cap;
	lead->ejobs_next = 0;
	return HMR_GPU_OK;
}
}  // namespace

extern "C" int hmr_gpu_enc_export_pictures_device(hmr_gpu_enc **encs, int n, const hmr_gpu_picture *pics, const int *slots, uint64_t *dev_ssd, void *consumer_stream)
{
	static const char *const fn = "hmr_gpu_enc_export_pictures_device";
	static_assert(EGRESS_MAX_JOBS == BATCH_MAX, "an export call follows a batch call");
	if (!encs || n < 1 || n > EGRESS_MAX_JOBS) {
		hmr_set_error("%s: needs 1 .. %d encoders (n = %d)", fn, EGRESS_MAX_JOBS, n);
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
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		if (!e) return egress_refuse(fn, i, "the encoder is NULL");
		if (e->ctx->device != encs[0]->ctx->device) return egress_refuse(fn, i, "the encoder is on another device than the call's first");
		if (!e->has_picture) return egress_refuse(fn, i, "the encoder has not encoded a picture yet");
		if (slots && (slots[i] < 0 || slots[i] >= (int)e->src.size())) return egress_refuse(fn, i, "the slot does not exist");
		if (slots && e->seq.width > EGRESS_MAX_WIDTH) return egress_refuse(fn, i, "sums are made for pictures up to 8192 samples wide");
		if (pics) {
			const int rc = hmr_gpu_picture_check(&pics[i], e->seq.width, e->seq.height);
			if (rc) {
				const std::string why = hmr_gpu_last_error();
				return egress_refuse(fn, i, why.c_str());
			}
		}
	}
	const int device = encs[0]->ctx->device;
	HIP_TRY(hipSetDevice(device));
	if (pics) {
		static const char *const names[3] = {"plane[0]", "plane[1]", "plane[2]"};
		for (int i = 0; i < n; i++)
			for (int c = 0; c < (pics[i].format == HMR_GPU_PIC_NV12 ? 2 : 3); c++)
				if (!on_device(pics[i].plane[c], device)) return egress_not_device(fn, i, names[c], device);
	}
	if (dev_ssd && (!on_device(dev_ssd, device) || !on_device(dev_ssd + 3 * (size_t)n - 1, device))) return egress_not_device(fn, 0, "dev_ssd", device);
	hmr_gpu_enc *lead = encs[0];
	hipStream_t st = lead->ctx->stream, consumer = (hipStream_t)consumer_stream;
	int rc = egress_prepare(lead, n);
	if (rc) return rc;
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		if (e->ev_pic_done) continue;
		HIP_TRY(hipEventCreateWithFlags(&e->ev_pic_done, hipEventDisableTiming));
		HIP_TRY(hipEventCreateWithFlags(&e->ev_own_done, hipEventDisableTiming));
	}
	const int turn = lead->ejobs_next;
	lead->ejobs_next = (turn + 1) % INGEST_RING;
	HIP_TRY(hipEventSynchronize(lead->ev_ejobs[turn]));      // (the launch of INGEST_RING calls ago: over long since; an event never recorded counts as complete)
	EgressJob *jobs = lead->h_ejobs + (size_t)turn * lead->ejobs_cap;
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		const Seq &s = e->seq;
		static_assert(sizeof(jobs[i].dst[0]) == sizeof(pics[i].plane[0]), "pointers");
		EgressJob &j = jobs[i];
		for (int c = 0; c < 3; c++) {
			j.rec[c] = plane0(e, e->cur, c);
			j.src[c] = slots ? e->src[slots[i]].p[c] : nullptr;
			j.dst[c] = pics ? const_cast<uint8_t *>(pics[i].plane[c]) : nullptr;      // (as the output descriptor: the call writes through the plane pointers)
			j.pitch[c] = pics ? pics[i].pitch[c] : 0;
		}
		j.ssd = dev_ssd ? dev_ssd + 3 * (size_t)i : nullptr;
		j.stride_y = s.stride_y; j.stride_c = s.stride_c;
		j.src_stride_y = s.src_stride_y; j.src_stride_c = s.src_stride_c;
		j.width = s.width; j.height = s.height;
		j.format = pics ? pics[i].format : HMR_GPU_PIC_I420; j.reserved = 0;
	}
	// behind the consumer (its work on the output memory and on dev_ssd), behind the launches that wrote the final pictures, behind what the encoders' own streams hold
	// (loads into the slots); every distinct stream once
	std::vector<hipStream_t> others(1, consumer);
	std::unordered_set<hipStream_t> seen = {consumer, st};
	HIP_TRY(hipEventRecord(lead->ev_consumer, consumer));
	if (consumer != st) HIP_TRY(hipStreamWaitEvent(st, lead->ev_consumer, 0));
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		const hipStream_t wrote[2] = {e->pic_stream, e->ctx->stream};
		hipEvent_t const ev[2] = {e->ev_pic_done, e->ev_own_done};
		for (int k = 0; k < 2; k++) {
			if (!seen.insert(wrote[k]).second) continue;
			others.push_back(wrote[k]);
			// a stream with nothing in flight has nothing to queue behind (calls on one encoder come from one host thread at a time: nobody is adding to it now);
			// the query is far cheaper than an event and a wait, and after an encode call most of a batch's streams are idle
			if (hipStreamQuery(wrote[k]) == hipSuccess) continue;
			(void)hipGetLastError();
			HIP_TRY(hipEventRecord(ev[k], wrote[k]));
			HIP_TRY(hipStreamWaitEvent(st, ev[k], 0));
		}
	}
	if (dev_ssd) HIP_TRY(hipMemsetAsync(dev_ssd, 0, 3 * (size_t)n * sizeof(uint64_t), st));
	if ((rc = hmr_egress_launch(st, jobs, lead->d_ejobs, n))) return rc;
	HIP_TRY(hipEventRecord(lead->ev_ejobs[turn], st));
	HIP_TRY(hipEventRecord(lead->ev_egressed, st));
	// the consumer reads the output behind the egress; a later encode call rewrites the final picture, a later load the slot: those streams go on behind it too
	for (hipStream_t w : others)
		if (w != st) HIP_TRY(hipStreamWaitEvent(w, lead->ev_egressed, 0));
	return HMR_GPU_OK;
}

extern "C" int hmr_gpu_enc_export_picture_device(hmr_gpu_enc *enc, const hmr_gpu_picture *pic, int slot, uint64_t *dev_ssd, void *consumer_stream)
{
	return hmr_gpu_enc_export_pictures_device(&enc, 1, pic, slot >= 0 ? &slot : nullptr, dev_ssd, consumer_stream);
}
