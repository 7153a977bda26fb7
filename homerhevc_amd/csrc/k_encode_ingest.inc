// Host side of the frame encoder, part 3 (included by k_encode.hip): pictures that already lie in device memory (include/homer_gpu.h section 12d).  One call converts
// the pictures of up to INGEST_MAX_JOBS encoders into their picture slots with one launch of k_ingest (k_ingest.hip) on the FIRST encoder's stream; events order it
// behind the producer's stream and in front of the other encoders' streams and of whatever the producer queues next.  The host waits for nothing.
namespace {
int ingest_refuse(const char *fn, int i, const char *what)
{
	hmr_set_error("%s: picture %d: %s", fn, i, what);
	return HMR_GPU_ERR_ARG;
}
// the lead's job tables and events, made when it first leads a call (or a larger one: the work queued with the old tables is waited for)
int ingest_prepare(hmr_gpu_enc *lead, int n)
{
	if (!lead->ev_produced) {
		HIP_TRY(hipEventCreateWithFlags(&lead->ev_produced, hipEventDisableTiming));
		HIP_TRY(hipEventCreateWithFlags(&lead->ev_ingested, hipEventDisableTiming));
		for (hipEvent_t &ev : lead->ev_jobs) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
	}
	if (n <= lead->jobs_cap) return HMR_GPU_OK;
	HIP_TRY(hipStreamSynchronize(lead->ctx->stream));
	if (lead->h_jobs) (void)hipHostFree(lead->h_jobs);
	if (lead->d_jobs) (void)hipFree(lead->d_jobs);
	lead->h_jobs = lead->d_jobs = nullptr;
	lead->jobs_cap = 0;
	const int cap = n == 1 ? 1 : INGEST_MAX_JOBS;
	HIP_TRY(hipHostMalloc((void **)&lead->h_jobs, (size_t)INGEST_RING * cap * sizeof(IngestJob), hipHostMallocDefault));
	HIP_TRY(hipMalloc((void **)&lead->d_jobs, (size_t)cap * sizeof(IngestJob)));
	lead->jobs_cap = cap;
	lead->jobs_next = 0;
	return HMR_GPU_OK;
}
}  // namespace

extern "C" int hmr_gpu_enc_load_sources_device(hmr_gpu_enc **encs, int n, const int *slots, const hmr_gpu_picture *pics, void *producer_stream)
{
	static const char *const fn = "hmr_gpu_enc_load_sources_device";
	static_assert(INGEST_MAX_JOBS == BATCH_MAX, "a load call feeds a batch call");
	if (!encs || !slots || !pics || n < 1 || n > INGEST_MAX_JOBS) {
		hmr_set_error("%s: needs 1 .. %d encoders with their slots and pictures (n = %d)", fn, INGEST_MAX_JOBS, n);
		return HMR_GPU_ERR_ARG;
	}
	for (int i = 0; i < n; i++) {
		if (!encs[i]) return ingest_refuse(fn, i, "the encoder is NULL");
		if (slots[i] < 0 || slots[i] > 4096) return ingest_refuse(fn, i, "the slot is outside 0 .. 4096");
		if (encs[i]->ctx->device != encs[0]->ctx->device) return ingest_refuse(fn, i, "the encoder is on another device than the call's first");
	}
	{
		// the same (encoder, slot) twice: two pictures into one slot in one launch would leave a mix of them
		std::vector<std::pair<hmr_gpu_enc *, int>> seen(n);
		for (int i = 0; i < n; i++) seen[i] = {encs[i], slots[i]};
		std::sort(seen.begin(), seen.end());
		if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) {
			hmr_set_error("%s: the same encoder and slot twice in one call", fn);
			return HMR_GPU_ERR_ARG;
		}
	}
	const int device = encs[0]->ctx->device;
	for (int i = 0; i < n; i++) {
		const int rc = hmr_gpu_picture_check(&pics[i], encs[i]->seq.width, encs[i]->seq.height);
		if (rc) {
			const std::string why = hmr_gpu_last_error();
			return ingest_refuse(fn, i, why.c_str());
		}
	}
	HIP_TRY(hipSetDevice(device));
	for (int i = 0; i < n; i++)
		for (int c = 0; c < (pics[i].format == HMR_GPU_PIC_NV12 ? 2 : 3); c++) {
			hipPointerAttribute_t attr;
			memset(&attr, 0, sizeof attr);
			if (hipPointerGetAttributes(&attr, pics[i].plane[c]) != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != device) {
				(void)hipGetLastError();
				hmr_set_error("%s: picture %d: plane[%d] is not device memory of device %d", fn, i, c, device);
				return HMR_GPU_ERR_ARG;
			}
		}
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		while ((int)e->src.size() <= slots[i]) {
			SrcSlot sl;
			for (int c = 0; c < 3; c++) DEV_ALLOC(sl.p[c], e->src_elems[c]);
			e->src.push_back(sl);
		}
	}
	hmr_gpu_enc *lead = encs[0];
	hipStream_t st = lead->ctx->stream, producer = (hipStream_t)producer_stream;
	int rc = ingest_prepare(lead, n);
	if (rc) return rc;
	const int turn = lead->jobs_next;
	lead->jobs_next = (turn + 1) % INGEST_RING;
	HIP_TRY(hipEventSynchronize(lead->ev_jobs[turn]));      // (the launch of INGEST_RING calls ago: over long since; an event never recorded counts as complete)
	IngestJob *jobs = lead->h_jobs + (size_t)turn * lead->jobs_cap;
	for (int i = 0; i < n; i++) {
		const hmr_gpu_enc *e = encs[i];
		IngestJob &j = jobs[i];
		for (int c = 0; c < 3; c++) {
			j.src[c] = pics[i].plane[c];
			j.pitch[c] = pics[i].pitch[c];
			j.dst[c] = e->src[slots[i]].p[c];
		}
		j.stride_y = e->seq.src_stride_y; j.stride_c = e->seq.src_stride_c;
		j.width = e->seq.width; j.height = e->seq.height;
		j.format = pics[i].format; j.reserved = 0;
	}
	// the pictures are complete when what the producer's stream holds now has run
	HIP_TRY(hipEventRecord(lead->ev_produced, producer));
	HIP_TRY(hipStreamWaitEvent(st, lead->ev_produced, 0));
	if ((rc = hmr_ingest_launch(st, jobs, lead->d_jobs, n))) return rc;
	HIP_TRY(hipEventRecord(lead->ev_jobs[turn], st));
	HIP_TRY(hipEventRecord(lead->ev_ingested, st));
	// every other encoder's stream (an encode call starts there: set-up copies, ev_ready) and the producer's (it may write the pictures again) go on behind the ingest
	std::vector<hipStream_t> waiting(1, producer);
	for (int i = 1; i < n; i++) waiting.push_back(encs[i]->ctx->stream);
	std::sort(waiting.begin(), waiting.end());
	waiting.erase(std::unique(waiting.begin(), waiting.end()), waiting.end());
	for (hipStream_t w : waiting)
		if (w != st) HIP_TRY(hipStreamWaitEvent(w, lead->ev_ingested, 0));
	return HMR_GPU_OK;
}

extern "C" int hmr_gpu_enc_load_source_device(hmr_gpu_enc *enc, int slot, const hmr_gpu_picture *pic, void *producer_stream)
{
	return hmr_gpu_enc_load_sources_device(&enc, 1, &slot, pic, producer_stream);
}
