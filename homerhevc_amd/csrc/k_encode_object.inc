// Host side of the frame encoder, part 1 (included by k_encode.hip: one translation unit with the kernels it launches): the encoder object (hmr_gpu_enc) - device
// memory, frame set-up, the launches of one picture, the engine objects' reference export / import - and the per-frame entry points of include/homer_gpu.h section 12.
// page-locked host memory for what comes back from the device every frame (records and levels: 11 MB per 1080p frame; a pageable target is copied through a
// staging buffer at a fraction of the link's rate)
template <class T>
struct PinnedAlloc {
	typedef T value_type;
	PinnedAlloc() = default;
	template <class U> PinnedAlloc(const PinnedAlloc<U> &) {}
	T *allocate(size_t n)
	{
		void *p = nullptr;
		if (hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) != hipSuccess) throw std::bad_alloc();
		return (T *)p;
	}
	void deallocate(T *p, size_t) { (void)hipHostFree(p); }
	template <class U> bool operator==(const PinnedAlloc<U> &) const { return true; }
	template <class U> bool operator!=(const PinnedAlloc<U> &) const { return false; }
};

// The phase planes (124 MB for a 1080p picture) are needed from the start of a P frame's CTU stage to its end.  An encoder object borrows a set for that
// time from a per-process pool instead of owning one: hundreds of sequences can be resident on a GPU (an engine ring keeps an engine object of EVERY
// sequence on every GPU) while only the pictures of the running step need planes.
struct PlaneSet { uint8_t *y = nullptr, *c[2] = {nullptr, nullptr}; size_t bytes_y = 0, bytes_c = 0; int device = 0; };
struct PlanePool {
	std::mutex m;
	std::vector<PlaneSet> free_sets;
	int acquire(int device, size_t by, size_t bc, PlaneSet *out)
	{
		{
			std::lock_guard<std::mutex> lk(m);
			for (size_t i = 0; i < free_sets.size(); i++)
				if (free_sets[i].device == device && free_sets[i].bytes_y == by && free_sets[i].bytes_c == bc) {
					*out = free_sets[i];
					free_sets.erase(free_sets.begin() + (long)i);
					return HMR_GPU_OK;
				}
		}
		PlaneSet p;
		p.device = device; p.bytes_y = by; p.bytes_c = bc;
		if (hipMalloc((void **)&p.y, by) != hipSuccess || hipMalloc((void **)&p.c[0], bc) != hipSuccess || hipMalloc((void **)&p.c[1], bc) != hipSuccess) {
			(void)hipGetLastError();
			if (p.y) (void)hipFree(p.y);
			if (p.c[0]) (void)hipFree(p.c[0]);
			if (p.c[1]) (void)hipFree(p.c[1]);
			hmr_set_error("phase planes: out of device memory (%zu bytes per picture)", by + 2 * bc);
			return HMR_GPU_ERR_HIP;
		}
		*out = p;
		return HMR_GPU_OK;
	}
	void release(const PlaneSet &p)
	{
		std::lock_guard<std::mutex> lk(m);
		free_sets.push_back(p);
	}
	// the pool keeps the sets of destroyed encoders for the next ones (a batch of 180 sequences allocates 38 GB of them once); when the last encoder is gone they
	// go back to the device
	int live = 0;
	void encoder_created() { std::lock_guard<std::mutex> lk(m); live++; }
	void encoder_destroyed()
	{
		std::lock_guard<std::mutex> lk(m);
		if (--live > 0) return;
		for (PlaneSet &p : free_sets) {
			(void)hipSetDevice(p.device);
			(void)hipFree(p.y); (void)hipFree(p.c[0]); (void)hipFree(p.c[1]);
		}
		free_sets.clear();
	}
};
PlanePool g_plane_pool;
struct hmr_gpu_enc {
	hmr_gpu_ctx *ctx;
	HostCfg cfg;
	// evaluations on a stale prediction window (quirk Q12, hmr_gpu_enc_stale_predictions): of the last picture (-1: none encoded yet), of all pictures
	long stale_last = -1, stale_total = 0;
	void note_stale_predictions(uint32_t n) { stale_last = (long)n; stale_total += (long)n; }
	Seq seq;
	HostState st;
	FrameCtx f;
	EncDev d;
	Seq *d_seq;
	FrameCtx *d_frame;
	Geo *d_geo;
	std::vector<Geo> geo;
	std::vector<SrcSlot> src;
	int16_t *d_pic[2][3], *d_pre[3], *d_rec[3];   // final pictures (current / reference), the deblocked picture, the reconstruction before the loop filters
	// post-decision stage (enc_post.h)
	PostRow *d_rows = nullptr;
	RowEnt *d_ent = nullptr;
	uint8_t *d_bs = nullptr;
	uint32_t *d_cumbits = nullptr;
	double *d_sao_tab = nullptr;         // [2 slice types: P, I][52][2]
	int *d_post_err = nullptr;
	// RD_FULL: the replay of the reference's coder objects (enc_rc.h), the states after every coded CTU of this frame and the one before, the table of the frame
	RdCtxSim rdsim[MAX_ENGINES];      // (an engine's coder objects are its own: hmr_encoder_lib.c:1096; an object that is ONE engine uses [0])
	uint8_t *d_ctx_ring = nullptr, *d_rd_init = nullptr;      // (ring: frame f in slot f mod RD_RING; d_rd_init: [all-zero | the slices' initial states per slot] x RD_CTX_BYTES)
	int *d_rd_src = nullptr;
	uint8_t h_rd_init[(1 + RD_RING) * RD_CTX_BYTES] = {0};
	uint16_t *d_rc_need = nullptr;       // rate control: the CTUs of each row that are coded when a wavefront step starts (enc_rc.h rc_need_table)
	RcFrame *d_rc_dyn = nullptr;
	int row_cap = 0;
	std::vector<RowEnt> h_ent;
	std::vector<uint8_t, PinnedAlloc<uint8_t>> h_bs;
	PlaneSet chain_planes2;          // (the set of its frame before: the object that ends a chain holds the planes the chain's first frame predicts from while its own S tasks write the next)
	PlaneSet chain_planes;           // overlapping frames (hmr_gpu_enc_encode_chain): the phase planes of THIS object's final picture, written by the S tasks of its CTU launch
	PlaneSet planes;                 // phase planes of the reference picture (k_subpel.hip: 16 luma, 2 x 64 chroma), borrowed from g_plane_pool for the CTU stage of a P frame
	size_t src_elems[3], pic_elems[3];
	uint8_t *d_bytes;              // staging for 8-bit planes (one 4:2:0 picture)
	// raster unit arrays of the filters, SAO statistics and parameters
	int units_stride, units_rows;
	int16_t *d_mvx, *d_mvy;
	int8_t *d_ref;
	uint8_t *d_qp, *d_flags;
	uint8_t *d_public;                                 // the CTUs' side-info records, packed for the download
	// host side of the entropy stage
	std::vector<uint8_t, PinnedAlloc<uint8_t>> h_public;
	std::vector<int16_t, PinnedAlloc<int16_t>> h_coeff;
	hipEvent_t ev_frame = nullptr, ev_ready = nullptr, ev_batch0 = nullptr, ev_batch1 = nullptr;   // (the batch launch has events of its own: frame_finish re-records the context's)   // start of the frame on the encoder's stream; its CTU stage may be launched
	int n_cus = 0;
	uint8_t *d_stage = nullptr, *h_stage = nullptr;      // batch: the packed sub-streams of all sequences (k_pack_streams), on the device and page-locked on the host
	size_t stage_bytes = 0;
	void *d_batch = nullptr;                             // (lead encoder) the EncDev records of a launch's pictures
	// pipelined batch (lead encoder): the step whose access units are still to be delivered
	bool pending = false;
	std::vector<hmr_gpu_enc *> pend_encs;
	std::vector<size_t> pend_off;                        // where each sequence's sub-streams lie in the staging buffer
	std::vector<std::vector<uint32_t>> pend_rows;        // and the bytes of each of its rows
	size_t *h_offs = nullptr;                            // (page-locked: k_pack_streams reads it)
	size_t pend_total = 0;
	hipStream_t copy_stream = nullptr;
	uint32_t *d_gather = nullptr, *h_gather = nullptr;   // per picture of a launch: the frame's counters and the CTUs' distortions
	size_t gather_words = 0;
	int record_words = 0;                                // (gather_pitch of the last launch)
	// (every encoder of the batch)
	bool awaiting_delivery = false;                      // its last frame's access unit has not been coded yet
	FrameCtx f_pending;                                  // that frame's parameters (e->f moves on with the next set_frame)
	hipEvent_t ev_decided = nullptr;                     // (lead) the batch's SAO decisions are made
	FrameCtx *d_frames = nullptr, *h_frames = nullptr;   // (lead) the frame parameters of a batch's pictures, on the device and page-locked on the host
	EncDev *h_devs = nullptr;                            // (lead) their EncDev records, page-locked
	hipStream_t plane_stream[2] = {nullptr, nullptr};    // (lead) side streams for the chroma phase planes of a batch
	hipEvent_t ev_plane[3] = {nullptr, nullptr, nullptr};
	int *d_pool_state = nullptr;                         // k_encode_pool: per picture of the launch the open step and the steps' ticket / done counters, then the finished-pictures counter
	WorkSlow *d_pool_slow = nullptr;                     // the pool workers' transform / decoded windows
	int pool_workers = 0;
	int last_pool_kernel = -1;                           // (lead) which kernel the last pool launch ran - 0: k_encode_pool_lat, 1: k_encode_pool, 2: k_encode_full; -1: none yet
	// picture conversion (picture_io.h, k_encode_picture_io.inc): the job tables and events, one ring per job type, of the picture launches this encoder leads - as the first
	// encoder of a load / export call, and alone in the host-memory entries (widen_packed, narrow_packed)
	PictureRings rings;
	// every encoder: whether d_pic[cur] holds an encoded frame's final picture, the stream whose work wrote it (its own, or the lead's of a batch or chain launch),
	// events for that stream and its own (an export call waits behind both)
	bool has_picture = false;
	hipStream_t pic_stream = nullptr;
	hipEvent_t ev_pic_done = nullptr, ev_own_done = nullptr;
	EntropyState es;
	// engines (enc_host.h): the persistent state of each engine this object runs - engine k = frames k, k + E, ... - swapped into d at set_frame
	CtuInfo *d_ctus_eng[MAX_ENGINES] = {nullptr};
	uint8_t *d_rowstate_eng[MAX_ENGINES] = {nullptr};
	int *d_seen_eng[MAX_ENGINES] = {nullptr};
	hmr_gpu_enc *twin_of = nullptr;   // hmr_gpu_enc_create_engine_twin: the object whose persistent engine state this one shares
	int local_engines = 1, engine_index = -1;     // engine_index >= 0: this object is ONE engine of st.engines (the others live elsewhere, hmr_gpu_enc_create_engine)
	int cur, lockstep;      // lockstep: the picture's CTUs run as tasks of k_encode_pool (the synchronous wavefront of wfpp_num_threads > 1, or `raster`)
	int raster = 0;
	float last_ms, last_total_ms;
	int last_passes, last_encodes;
};

namespace {
void release_planes(hmr_gpu_enc *e);
constexpr int REC_BYTES = 32 + 3 * 256 + 2 * 256 + 9 * 256 + 256 + 256 + 2048 + 2048 + 6144 * 2 + 6144 * 2 + 2 * 5 * 256;

int16_t *plane0(hmr_gpu_enc *e, int which, int comp)
{
	const Seq &s = e->seq;
	const int st = comp ? s.stride_c : s.stride_y, m = comp ? s.margin_c : s.margin_y;
	return e->d_pic[which][comp] + (size_t)m * st + m;
}

// device memory, cleared ON THE ENCODER'S STREAM: the stream is non-blocking, so a hipMemset (null stream) is not ordered against the work that follows on it -
// a picture slot allocated by hmr_gpu_enc_load_source could be cleared after the picture had been written into it (seen as an occasional different stream)
template <class T>
int dev_alloc(T **p, size_t n, hipStream_t st)
{
	HIP_TRY(hipMalloc((void **)p, n * sizeof(T)));
	HIP_TRY(hipMemsetAsync(*p, 0, n * sizeof(T), st));
	HIP_TRY(hipStreamSynchronize(st));   // (and a synchronous copy into the buffer, which runs on the null stream, must not overtake the clearing either)
	return HMR_GPU_OK;
}
#define DEV_ALLOC(p, n)                           \
	do {                                      \
		const int rc_ = dev_alloc(&(p), (n), e->ctx->stream); \
		if (rc_) return rc_;              \
	} while (0)

// e's final picture as picture_io.h's job builders take it, and as a picture slot is held: the planes at sample (0, 0); their strides are e->seq.stride_y / stride_c
SrcSlot final_planes(hmr_gpu_enc *e) { return SrcSlot{{plane0(e, e->cur, 0), plane0(e, e->cur, 1), plane0(e, e->cur, 2)}}; }
// a tightly packed I420 picture of e's size at `bytes` (luma pitch width, chroma pitch width / 2): the staging buffer d_bytes, a picture as it travels between GPUs
hmr_gpu_picture packed_picture(const hmr_gpu_enc *e, const uint8_t *bytes)
{
	const int64_t w = e->seq.width, h = e->seq.height;
	return hmr_gpu_picture{HMR_GPU_PIC_I420, 0, {bytes, bytes + w * h, bytes + w * h + (w / 2) * (h / 2)}, {w, w / 2, w / 2}};
}
// Queued on the encoder's own stream, nothing waited for: the packed picture at `bytes` (device memory) into the planes `dst` / e's final picture into one at `bytes`.
int widen_packed(hmr_gpu_enc *e, const uint8_t *bytes, int16_t *const dst[3], int stride_y, int stride_c)
{
	const IngestJob j = hmr_ingest_job(packed_picture(e, bytes), dst, stride_y, stride_c, e->seq.width, e->seq.height);
	return run_jobs(e->rings, e->ctx->stream, &j, 1, e->ctx->stream);
}
int narrow_packed(hmr_gpu_enc *e, uint8_t *bytes)
{
	const Seq &s = e->seq;
	const hmr_gpu_picture pic = packed_picture(e, bytes);
	const EgressJob j = hmr_egress_job(final_planes(e).p, s.stride_y, s.stride_c, &pic, nullptr, s.src_stride_y, s.src_stride_c, nullptr, s.width, s.height);
	return run_jobs(e->rings, e->ctx->stream, &j, 1, e->ctx->stream);
}

// a picture in host memory into the planes `dst`: the device path (k_ingest) plus the copy into the staging buffer and a synchronise
int load_planes(hmr_gpu_enc *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, int16_t *const dst[3], int stride_y, int stride_c)
{
	hipStream_t st = e->ctx->stream;
	const hmr_gpu_picture staged = packed_picture(e, e->d_bytes);
	const uint8_t *in[3] = {y, u, v};
	for (int c = 0; c < 3; c++)
		HIP_TRY(hipMemcpyAsync(const_cast<uint8_t *>(staged.plane[c]), in[c], (size_t)staged.pitch[c] * (c ? e->seq.height / 2 : e->seq.height), hipMemcpyHostToDevice, st));
	const int rc = widen_packed(e, e->d_bytes, dst, stride_y, stride_c);
	if (rc) return rc;
	HIP_TRY(hipStreamSynchronize(st));
	return HMR_GPU_OK;
}


// what a frame's CTU stage needs on the stream before its first launch
// the reference picture, interpolated once at every sub-sample phase: what motion search and compensation read (k_subpel.hip)
int reference_planes(hmr_gpu_enc *e, hipStream_t st)
{
	const Seq &s = e->seq;
	if (e->f.slice_type == SLICE_I) return HMR_GPU_OK;
	return hmr_subpel_planes_on(st, e->d_pic[e->cur ^ 1][0], e->d_pic[e->cur ^ 1][1], e->d_pic[e->cur ^ 1][2], s.stride_y, s.height + 2 * s.margin_y, s.stride_c,
				    s.height / 2 + 2 * s.margin_c, e->planes.y, e->planes.c[0], e->planes.c[1]);
}
int ctu_stage_prepare(hmr_gpu_enc *e, bool planes_elsewhere = false)
{
	const Seq &s = e->seq;
	hipStream_t st = e->ctx->stream;
	if (!e->lockstep)   // (the frame-start state CTUs are re-encoded from in the single-thread order)
		HIP_TRY(hipMemcpyAsync(e->d.ctus_start, e->d.ctus, sizeof(CtuInfo) * s.nctu, hipMemcpyDeviceToDevice, st));
	if (!planes_elsewhere) {
		const int rc = reference_planes(e, st);
		if (rc) return rc;
	}
	{
		static const int zero_counters[3] = {0, 0, -1};
		HIP_TRY(hipMemcpyAsync(e->d.counters, zero_counters, sizeof zero_counters, hipMemcpyHostToDevice, st));
	}
	if (e->lockstep) {
		HIP_TRY(hipMemsetAsync(e->d.progress, 0, sizeof(int) * s.hctu, st));
		HIP_TRY(hipMemsetAsync(e->d.row0_checked, 0, sizeof(int), st));
		HIP_TRY(hipMemsetAsync(e->d.prefix, 0, sizeof(uint32_t) * s.hctu * (s.wctu + 1), st));
	}
	HIP_TRY(hipMemsetAsync(e->d_rows, 0, sizeof(PostRow) * s.hctu, st));
	HIP_TRY(hipMemsetAsync(e->d_post_err, 0, sizeof(int) * 4, st));
	return HMR_GPU_OK;
}
int lockstep_run(hmr_gpu_enc *e);      // (behind k_gather_results)

// CTUs of a picture that can be decided at the same time: a wavefront step holds one CTU of every second column, so at most min(rows, (columns + 1) / 2); under rate
// control a step also waits for the entropy coder's progress (enc_rc.h), which about halves it.  Workers beyond what a launch can keep busy are not merely idle: every
// active worker runs slower the more of them share the chip's caches (a 2160p CBR batch of 32: 45 frames/s on 512 workers, 43 on 640, 30 on 1024)
static int pool_inflight(const Seq &s, int raster = 0)
{
	if (raster) return 3;      // (raster order: one CTU is decided at a time; two more workers for the post-decision tasks behind it)
	const int by_step = s.hctu < (s.wctu + 1) / 2 ? s.hctu : (s.wctu + 1) / 2;
	return s.bitrate_mode != 0 ? (by_step + 1) / 2 : by_step;
}
// the row-per-thread schedule of n pictures (their EncDev records already at lead->d_batch, `host` the copies they were made from) as ONE pool launch on `st`;
// rows_total: the sum of their pool_inflight(); needs_rd: one of them at least is RD_FULL
int launch_pool(hmr_gpu_enc *lead, const EncDev *host, int n, int rows_total, bool needs_rd, hipStream_t st)
{
	if (!lead->n_cus) HIP_TRY(hipDeviceGetAttribute(&lead->n_cus, hipDeviceAttributeMultiprocessorCount, lead->ctx->device));
	// a worker's LDS: without RD_FULL pictures in the launch the RD arrays at its end are left out (a fourth worker then fits a CU)
	const size_t lds_default = (size_t)lds_request(needs_rd);
	const size_t lds_bytes = getenv("HENC_LDS_BYTES") && (size_t)atoi(getenv("HENC_LDS_BYTES")) > lds_default ? (size_t)atoi(getenv("HENC_LDS_BYTES")) : lds_default;   // (experiment: a larger request keeps a CU to fewer workers)
	if (lds_bytes > 160 * 1024) {
		hmr_set_error("k_encode_pool: a worker's LDS request of %zu bytes (HENC_LDS_BYTES) is more than a CU has", lds_bytes);
		return HMR_GPU_ERR_ARG;
	}
	const int cap = lead->n_cus * workers_per_cu(lds_bytes);                  // what the LDS lets be resident; more would only queue behind
	int workers = rows_total < cap ? rows_total : cap;                        // (a picture never has more CTUs in flight than rows)
	if (workers < 1) workers = 1;
	if (getenv("HENC_POOL_WORKERS") && atoi(getenv("HENC_POOL_WORKERS")) > 0 && atoi(getenv("HENC_POOL_WORKERS")) < workers) workers = atoi(getenv("HENC_POOL_WORKERS"));      // (experiment)
	// at most one worker per CU: the latency kernel, whose helpers also run a CU's intra mode search under its inter evaluation (enc_common.h bg_post).  Otherwise the
	// throughput kernel, whose walk is compiled without full RDO (enc_platform.h WaveGrpLean) - or, with an RD_FULL picture in the launch, the generic kernel.
	const int kernel = workers <= lead->n_cus ? 0 : (needs_rd ? 2 : 1);
	if (kernel == 1)      // (set_frame gives the record of an RD_FULL picture, and no other, the sources of its bit estimates)
		for (int i = 0; i < n; i++)
			if (host[i].rd_src) {
				hmr_set_error("k_encode_pool: picture %d of the launch is RD_FULL, and this kernel's walk is compiled without full RDO (needs_rd was not set)", i);
				return HMR_GPU_ERR_ARG;
			}
	if (!lead->d_pool_state) HIP_TRY(hipMalloc((void **)&lead->d_pool_state, sizeof(int) * (BATCH_MAX * POOL_STRIDE + 4)));
	if (lead->pool_workers < workers) {
		if (lead->d_pool_slow) (void)hipFree(lead->d_pool_slow);
		lead->d_pool_slow = nullptr;
		lead->pool_workers = 0;
		HIP_TRY(hipMalloc((void **)&lead->d_pool_slow, sizeof(WorkSlow) * workers));
		HIP_TRY(hipMemsetAsync(lead->d_pool_slow, 0, sizeof(WorkSlow) * workers, st));
		lead->pool_workers = workers;
	}
	HIP_TRY(hipMemsetAsync(lead->d_pool_state, 0, sizeof(int) * (BATCH_MAX * POOL_STRIDE + 4), st));
	// the watchdog (100 MHz ticks): a launch is a second or two of work; a worker that finds nothing to do for this long gives up for everybody
	double watchdog_s = getenv("HENC_WATCHDOG_S") ? atof(getenv("HENC_WATCHDOG_S")) : 120.0;
	if (!(watchdog_s > 0)) watchdog_s = 120.0;
	const unsigned long long watchdog = (unsigned long long)(watchdog_s * 1e8);
	auto *const fn = kernel == 0 ? k_encode_pool_lat : (kernel == 1 ? k_encode_pool : k_encode_full);
	hipLaunchKernelGGL(fn, dim3(workers), dim3(ENC_THREADS), lds_bytes, st, (const EncDev *)lead->d_batch, n, lead->d_pool_state, lead->d_pool_state + BATCH_MAX * POOL_STRIDE,
			   lead->d_pool_slow, watchdog, (unsigned)lds_default);
	const hipError_t launched = hipGetLastError();
	if (launched != hipSuccess) {
		hmr_set_error("k_encode_pool: %s", hipGetErrorString(launched));
		return HMR_GPU_ERR_HIP;
	}
	lead->last_pool_kernel = kernel;
	return HMR_GPU_OK;
}

// the CTU decisions of the frame set up in e->f / e->d_frame: passes until the check finds nothing wrong
int run_ctu_passes(hmr_gpu_enc *e)
{
	if (e->lockstep) return lockstep_run(e);      // wfpp_num_threads > 1: the synchronous wavefront, one launch, nothing to verify - the picture's CTUs as a pool of tasks (k_encode_pool)
	const Seq &s = e->seq;
	hipStream_t st = e->ctx->stream;
	int rc = ctu_stage_prepare(e);
	if (rc) return rc;
	HIP_TRY(hipEventRecord(e->ctx->ev0, st));
	// wfpp_num_threads = 1: the single thread's order.  Row workers wait for the row above (progress[]), so every workgroup of the launch has to be resident
	// or the waiting ones spin for ever: a cooperative launch makes the runtime guarantee that - it fails at launch time when the grid does not fit (another
	// process on the GPU, a partition mode) instead of hanging.
	int pass = 0;
	for (;; pass++) {
		HIP_TRY(hipMemsetAsync(e->d.progress, 0, sizeof(int) * s.hctu, st));
		{
			EncDev dd = e->d;
			int pp = pass;
			void *args[] = {&dd, &pp};
			const hipError_t launched = hipLaunchCooperativeKernel((const void *)k_encode_ctus, dim3(s.hctu), dim3(ENC_THREADS), args, (unsigned)lds_request(true), st);
			if (launched != hipSuccess) {
				hmr_set_error("k_encode_ctus (%d row workers, cooperative): %s", s.hctu, hipGetErrorString(launched));
				return HMR_GPU_ERR_HIP;
			}
		}
		hipLaunchKernelGGL(k_sched_scan, dim3(1), dim3(320), 0, st, e->d);
		hipLaunchKernelGGL(k_sched_check, dim3(s.nctu), dim3(64), 0, st, e->d);
		HIP_TRY(hipGetLastError());
		int counters[3];
		HIP_TRY(hipMemcpyAsync(counters, e->d.counters, sizeof counters, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		e->last_encodes = counters[1];
		e->f.scene_cut_ctu = counters[2];
		if (counters[0] == 0) break;
		if (pass > s.nctu + 2) {
			hmr_set_error("hmr_gpu_enc: the CTU schedule did not converge");
			return HMR_GPU_ERR_HIP;
		}
	}
	hipLaunchKernelGGL(k_sched_finish, dim3(s.nctu), dim3(64), 0, st, e->d);
	HIP_TRY(hipMemcpyAsync(e->d.chain_start, e->d.chain_end, MODE_STATE_BYTES, hipMemcpyDeviceToDevice, st));
	HIP_TRY(hipMemcpyAsync(e->d_frame, &e->f, sizeof(FrameCtx), hipMemcpyHostToDevice, st));      // (scene_cut_ctu as the passes found it)
	HIP_TRY(hipFuncSetAttribute((const void *)k_post_frame, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PostScratch)));
	hipLaunchKernelGGL(k_post_frame, dim3(s.hctu < 32 ? s.hctu : 32), dim3(64), sizeof(PostScratch), st, e->d);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(e->ctx->ev1, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipEventElapsedTime(&e->last_ms, e->ctx->ev0, e->ctx->ev1));
	e->last_passes = pass + 1;
	release_planes(e);
	return HMR_GPU_OK;
}

int set_frame(hmr_gpu_enc *e, int slot, int image_type, double avg_dist, bool upload = true, bool chain = false)
{
	const Seq &s = e->seq;
	e->cur ^= 1;
	e->has_picture = true;
	e->pic_stream = e->ctx->stream;      // (a batch or chain launch names its lead's stream after this)
	{
		const int k = e->local_engines > 1 ? e->st.num_encoded_frames % e->local_engines : 0;
		e->d.ctus = e->d_ctus_eng[k];
		e->d.rowstate = e->d_rowstate_eng[k];
		e->d.thread_seen = e->d_seen_eng[k];
	}
	begin_frame(s, e->st, image_type, e->f);
	if (avg_dist >= 0) e->f.avg_dist = avg_dist;
	e->f.lockstep = e->lockstep && !e->raster;      // (the decision code's flag: the synchronous wavefront's rules for "after the scene cut")
	for (int c = 0; c < 3; c++) {
		e->f.src[c] = e->src[slot].p[c];
		e->f.ref[c] = plane0(e, e->cur ^ 1, c);
		e->f.rec[c] = e->d_rec[c] + (size_t)(c ? s.margin_c : s.margin_y) * (c ? s.stride_c : s.stride_y) + (c ? s.margin_c : s.margin_y);
		e->d.post.fin[c] = plane0(e, e->cur, c);
	}
	e->d.post.sao_lambda = e->d_sao_tab + (e->f.slice_type == SLICE_I ? 104 : 0);
	e->d.post.ctx_after = nullptr;
	if (s.rd_mode == RDM_FULL) {
		// which coder states each CTU's estimates copy this frame (enc_rc.h RdCtxSim), as a table for the CTU kernel
		std::vector<RdCtxVersion> src;
		e->rdsim[e->local_engines > 1 ? e->f.num_encoded_frames % e->local_engines : 0].frame(e->f.num_encoded_frames, src, e->raster != 0);
		std::vector<int> codes(s.nctu);
		for (int n = 0; n < s.nctu; n++) {
			const RdCtxVersion v = src[n];
			if (v.frame > e->f.num_encoded_frames || (v.frame >= 0 && v.frame <= e->f.num_encoded_frames - RD_RING)) {
				hmr_set_error("RD_FULL: CTU %d copies coder states of frame %d in frame %d (the states of %d frames are kept)", n, v.frame, e->f.num_encoded_frames, RD_RING);
				return HMR_GPU_ERR_ARG;
			}
			const int slot = v.frame < 0 ? 0 : v.frame % RD_RING;
			codes[n] = v.frame < 0 ? 0 : (v.k == 0 ? (1 << 28) | (slot << 24) : (3 << 28) | (slot << 24) | (v.row * s.wctu + v.k - 1));
		}
		const int slot_now = e->f.num_encoded_frames % RD_RING;
		for (int i = 0; i < CTX_TOTAL; i++) e->h_rd_init[(1 + slot_now) * RD_CTX_BYTES + i] = Cabac::init_state(e->f.slice_type, e->f.qp, i);
		HIP_TRY(hipMemcpyAsync(e->d_rd_src, codes.data(), sizeof(int) * s.nctu, hipMemcpyHostToDevice, e->ctx->stream));      // (pageable sources: copied before the call returns)
		HIP_TRY(hipMemcpyAsync(e->d_rd_init, e->h_rd_init, sizeof e->h_rd_init, hipMemcpyHostToDevice, e->ctx->stream));
		e->d.post.ctx_after = e->d_ctx_ring + (size_t)slot_now * s.nctu * RD_CTX_BYTES;
		e->d.rd_src = e->d_rd_src;
		e->d.rd_init = e->d_rd_init;
		e->d.rd_ring = e->d_ctx_ring;
	}
	e->d.dep = -1;
	e->d.dep_full = 0;
	e->d.after = -1;
	e->d.next_frame = nullptr;
	e->d.post.planes[0] = e->d.post.planes[1] = e->d.post.planes[2] = nullptr;
	if (e->f.slice_type != SLICE_I && !chain) {
		if (!e->planes.y) {
			const int rc = g_plane_pool.acquire(e->ctx->device, (size_t)16 * s.plane_elems_y, (size_t)64 * s.plane_elems_c, &e->planes);
			if (rc) return rc;
		}
		e->f.sub_y = e->planes.y + (size_t)s.margin_y * 16 * s.stride_y + s.margin_y;       // (row-interleaved: a row of the picture is 16 / 64 rows of phases)
		e->f.sub_c[0] = e->planes.c[0] + (size_t)s.margin_c * 64 * s.stride_c + s.margin_c;
		e->f.sub_c[1] = e->planes.c[1] + (size_t)s.margin_c * 64 * s.stride_c + s.margin_c;
	}
	if (upload) HIP_TRY(hipMemcpyAsync(e->d_frame, &e->f, sizeof(FrameCtx), hipMemcpyHostToDevice, e->ctx->stream));      // (a batch uploads its frames' parameters in one copy)
	return HMR_GPU_OK;
}

// the CTU stage of the frame is over (its launch has been waited for): the planes go back to the pool
void release_planes(hmr_gpu_enc *e)
{
	if (e->planes.y) g_plane_pool.release(e->planes);
	e->planes = PlaneSet();
}

// the three planes of a picture to their copies in one launch (three device-to-device copies are three copy kernels on the stream)
__global__ __launch_bounds__(256) void k_copy_planes(const int16_t *s0, const int16_t *s1, const int16_t *s2, int16_t *d0, int16_t *d1, int16_t *d2, size_t n0, size_t n12)
{
	const int c = (int)blockIdx.y;
	const uint4 *s = (const uint4 *)(c == 0 ? s0 : (c == 1 ? s1 : s2));
	uint4 *d = (uint4 *)(c == 0 ? d0 : (c == 1 ? d1 : d2));
	const size_t n = (c == 0 ? n0 : n12) / 8;      // eight samples per thread and step (the planes' sizes are multiples of eight)
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) d[i] = s[i];
}

// the side-info records lie 68 KB apart inside the CTU records: packed on the device, then one linear copy to the host
__global__ void k_pack_public(const CtuInfo *ctus, uint32_t *out)
{
	const uint32_t *src = (const uint32_t *)(const CtuPublic *)(ctus + blockIdx.x);
	uint32_t *dst = out + (size_t)blockIdx.x * (sizeof(CtuPublic) / 4);
	for (int i = threadIdx.x; i < (int)(sizeof(CtuPublic) / 4); i += blockDim.x) dst[i] = src[i];
}
// single-thread order: the picture's evaluations on a stale prediction window (CtuInfo::n_stale_pred of each CTU's last encode), into the free slot of the error record
__global__ void k_sum_stale(const CtuInfo *ctus, int nctu, int *out)
{
	int n = 0;
	for (int c = threadIdx.x; c < nctu; c += blockDim.x) n += ctus[c].n_stale_pred;
	if (n) atomicAdd(out, n);
}
int download_public(hmr_gpu_enc *e)
{
	const Seq &s = e->seq;
	hipLaunchKernelGGL(k_sum_stale, dim3(1), dim3(256), 0, e->ctx->stream, (const CtuInfo *)e->d.ctus, s.nctu, e->d_post_err + 3);
	hipLaunchKernelGGL(k_pack_public, dim3(s.nctu), dim3(256), 0, e->ctx->stream, e->d.ctus, (uint32_t *)e->d_public);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(e->h_public.data(), e->d_public, sizeof(CtuPublic) * s.nctu, hipMemcpyDeviceToHost, e->ctx->stream));
	return HMR_GPU_OK;
}
}  // namespace

extern "C" int hmr_gpu_enc_record_bytes(void) { return REC_BYTES; }

static thread_local int g_serial_pool = 0;      // hmr_gpu_enc_create_serial_pool: the object being created runs wfpp_num_threads = 1 in the pool's raster schedule whatever its other settings
static int enc_create(hmr_gpu_ctx *ctx, const hmr_gpu_enc_cfg *cfg, int engine_index, hmr_gpu_enc **out)
{
	if (!ctx || !cfg || !out) return HMR_GPU_ERR_ARG;
	static_assert(sizeof(hmr_gpu_enc_cfg) == sizeof(HostCfg), "configuration layouts must match");
	static_assert(offsetof(CtuInfo, n_spec_reads) % 4 == 0 && sizeof(Node) % 4 == 0 && sizeof(Geo) % 2 == 0 && sizeof(Seq) % 4 == 0 && sizeof(FrameCtx) % 4 == 0 && sizeof(CtuPublic) % 4 == 0 && MODE_STATE_BYTES % 4 == 0, "word copies");
	hmr_gpu_enc *e = new hmr_gpu_enc();
	e->ctx = ctx;
	memcpy(&e->cfg, cfg, sizeof(HostCfg));
	const char *why = "";
	if (!make_seq(e->cfg, e->seq, &why)) {
		hmr_set_error("hmr_gpu_enc_create: configuration outside the built rows: %s", why);
		delete e;
		return HMR_GPU_ERR_ARG;
	}
	e->st.engines = clampi(e->cfg.num_enc_engines, 1, MAX_ENGINES);
	e->engine_index = engine_index;
	e->local_engines = engine_index >= 0 ? 1 : e->st.engines;
	if (e->st.engines > 1 && e->cfg.wfpp_num_threads < 2 && engine_index >= 0) {
		hmr_set_error("hmr_gpu_enc_create: configuration outside the built rows: num_enc_engines > 1 needs the row-per-thread schedule (wfpp_num_threads > 1)");
		delete e;
		return HMR_GPU_ERR_ARG;
	}
	if (engine_index >= e->st.engines) { delete e; return HMR_GPU_ERR_ARG; }
#if defined(HENC_NO_RDFULL)
	if (e->seq.rd_mode == RDM_FULL) {      // (the experiment build of enc_platform.h: no kernel of it carries full RDO)
		hmr_set_error("hmr_gpu_enc_create: this library was built with -DHENC_NO_RDFULL and cannot encode rd_mode RD_FULL");
		delete e;
		return HMR_GPU_ERR_ARG;
	}
#endif
	if (e->cfg.bitrate_mode != 0) host_rc_init(e->cfg, e->seq, e->st);
	g_plane_pool.encoder_created();      // (hmr_gpu_enc_destroy - also the guard's - takes it back)
	struct Guard {               // a failure further down (HIP_TRY / DEV_ALLOC return) frees what has been allocated so far
		hmr_gpu_enc *e;
		bool ok = false;
		~Guard() { if (!ok) hmr_gpu_enc_destroy(e); }
	} guard{e};
	e->seq.wide_min_n = 0;
	// One WPP thread: the single thread's order by guesses, verification and re-encode passes (k_encode_ctus) - except under rate control and RD_FULL, whose decisions
	// read the entropy coder's progress and states behind FINAL decisions (hmr_rate_control.c:266-282, hmr_arithmetic_encoding.c:2139): there the pool runs the
	// picture one CTU at a time in raster order (EncDev::raster), the post-decision tasks beside it on the launch's other workers.  Several engines in one object take that
	// schedule too (the engines' persistent state is swapped by set_frame, which the pool's launch follows); an object that is ONE engine needs wfpp_num_threads > 1 (above).
	e->raster = e->cfg.wfpp_num_threads <= 1 && (e->cfg.bitrate_mode != 0 || e->seq.rd_mode == RDM_FULL || g_serial_pool || e->st.engines > 1);
	e->lockstep = e->cfg.wfpp_num_threads > 1 || e->raster;
	const Seq &s = e->seq;
	HIP_TRY(hipSetDevice(ctx->device));
	e->geo.resize(NNODES);
	make_geo(e->geo.data());
	DEV_ALLOC(e->d_seq, 1);
	HIP_TRY(hipMemcpy(e->d_seq, &s, sizeof(Seq), hipMemcpyHostToDevice));
	DEV_ALLOC(e->d_frame, 1);
	DEV_ALLOC(e->d_geo, NNODES);
	HIP_TRY(hipMemcpy(e->d_geo, e->geo.data(), sizeof(Geo) * NNODES, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(henc_geo_table), e->geo.data(), sizeof(Geo) * NNODES));   // (the same tree for every encoder: 64 x 64 CTUs, prediction depth 4)
	DEV_ALLOC(e->d.ctus, s.nctu);
	if (e->cfg.wfpp_num_threads <= 1) DEV_ALLOC(e->d.ctus_start, s.nctu);   // (the frame-start state CTUs are re-encoded from: single-thread order only)
	{
		std::vector<CtuInfo> init(s.nctu);
		memset((void *)init.data(), 0, sizeof(CtuInfo) * s.nctu);
		for (auto &c : init) memset(c.mv_ref_idx, -1, sizeof c.mv_ref_idx);
		HIP_TRY(hipMemcpy(e->d.ctus, init.data(), sizeof(CtuInfo) * s.nctu, hipMemcpyHostToDevice));
		e->d_ctus_eng[0] = e->d.ctus;
		for (int k = 1; k < e->local_engines; k++) {
			DEV_ALLOC(e->d_ctus_eng[k], s.nctu);
			HIP_TRY(hipMemcpy(e->d_ctus_eng[k], init.data(), sizeof(CtuInfo) * s.nctu, hipMemcpyHostToDevice));
		}
	}
	if (e->cfg.wfpp_num_threads <= 1) DEV_ALLOC(e->d.work_slow, s.hctu);      // (the pool has its workers' windows: lead->d_pool_slow)
	HIP_TRY(hipFuncSetAttribute((const void *)k_encode_ctus, hipFuncAttributeMaxDynamicSharedMemorySize, lds_request(true)));
	HIP_TRY(hipFuncSetAttribute((const void *)k_encode_pool, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
	HIP_TRY(hipFuncSetAttribute((const void *)k_encode_pool_lat, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
	HIP_TRY(hipFuncSetAttribute((const void *)k_encode_full, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
	HIP_TRY(hipEventCreate(&e->ev_frame));
	HIP_TRY(hipEventCreate(&e->ev_ready));
	HIP_TRY(hipEventCreate(&e->ev_batch0));
	HIP_TRY(hipEventCreate(&e->ev_batch1));
	HIP_TRY(hipEventCreateWithFlags(&e->ev_decided, hipEventDisableTiming));
	DEV_ALLOC(e->d.coeff, (size_t)6144 * s.nctu);
	DEV_ALLOC(e->d.progress, s.hctu);
	DEV_ALLOC(e->d.prefix, (size_t)s.hctu * (s.wctu + 1));
	DEV_ALLOC(e->d.prof, (size_t)s.hctu * PF_COUNT + (size_t)s.nctu * 4);   // + per CTU: 100 MHz timestamps of wait start, encode start, first use of the intra share, end
	DEV_ALLOC(e->d.guess, (size_t)s.nctu * MODE_STATE_BYTES);
	DEV_ALLOC(e->d.truth, (size_t)s.nctu * MODE_STATE_BYTES);
	DEV_ALLOC(e->d.outtok, (size_t)s.nctu * MODE_STATE_BYTES);
	DEV_ALLOC(e->d.chain_start, MODE_STATE_BYTES);
	DEV_ALLOC(e->d.chain_end, MODE_STATE_BYTES);
	DEV_ALLOC(e->d.valid, s.nctu);
	DEV_ALLOC(e->d.dirty, s.nctu);
	DEV_ALLOC(e->d.hash, s.nctu);
	DEV_ALLOC(e->d.intra_before, s.nctu);
	DEV_ALLOC(e->d.used_intra, s.nctu);
	DEV_ALLOC(e->d.used_parts, s.nctu);
	DEV_ALLOC(e->d.counters, 4);
	DEV_ALLOC(e->d.rowstate, (size_t)s.hctu * ROW_STATE_BYTES);
	DEV_ALLOC(e->d.thread_seen, 64);
	e->d_rowstate_eng[0] = e->d.rowstate;
	e->d_seen_eng[0] = e->d.thread_seen;
	for (int k = 1; k < e->local_engines; k++) {
		DEV_ALLOC(e->d_rowstate_eng[k], (size_t)s.hctu * ROW_STATE_BYTES);
		DEV_ALLOC(e->d_seen_eng[k], 64);
	}
	DEV_ALLOC(e->d.row0_checked, 1);
	for (int c = 0; c < 3; c++) {
		e->src_elems[c] = (size_t)(c ? s.src_stride_c : s.src_stride_y) * (c ? s.height / 2 : s.height);
		e->pic_elems[c] = (size_t)(c ? s.stride_c : s.stride_y) * ((c ? s.height / 2 : s.height) + 2 * (c ? s.margin_c : s.margin_y));
		for (int k = 0; k < 2; k++) DEV_ALLOC(e->d_pic[k][c], e->pic_elems[c]);
		DEV_ALLOC(e->d_pre[c], e->pic_elems[c]);
		DEV_ALLOC(e->d_rec[c], e->pic_elems[c]);
	}
	{
		// the post-decision stage: row progress, the rows' CABAC coders and sub-streams (CTU_STREAM_BOUND per CTU, enc_post.h: the most any content can take;
		// a sub-stream that runs out of room is still an error return, not a truncated stream), the SAO Lagrange multipliers of both slice types by QP
		e->row_cap = s.wctu * CTU_STREAM_BOUND;
		DEV_ALLOC(e->d_rows, s.hctu);
		DEV_ALLOC(e->d_ent, s.hctu);
		DEV_ALLOC(e->d_bs, (size_t)e->row_cap * s.hctu);
		DEV_ALLOC(e->d_cumbits, s.nctu);
		DEV_ALLOC(e->d_sao_tab, 2 * 52 * 2);
		DEV_ALLOC(e->d_post_err, 4 + 2 * 16 + 4);
		double tab[2][104];
		sao_lambda_table(s, SLICE_P, tab[0]);
		sao_lambda_table(s, SLICE_I, tab[1]);
		HIP_TRY(hipMemcpy(e->d_sao_tab, tab, sizeof tab, hipMemcpyHostToDevice));
		e->h_ent.resize(s.hctu);
		DEV_ALLOC(e->d_rc_dyn, 1);
		if (s.rd_mode == RDM_FULL) {
			for (auto &sim : e->rdsim) sim.init(e->cfg.wfpp_num_threads > 1 ? e->cfg.wfpp_num_threads : 1, s.wctu, s.hctu, s.sao);
			DEV_ALLOC(e->d_ctx_ring, (size_t)RD_RING * s.nctu * RD_CTX_BYTES);
			HIP_TRY(hipMemset(e->d_ctx_ring, 0, (size_t)RD_RING * s.nctu * RD_CTX_BYTES));
			DEV_ALLOC(e->d_rd_init, (1 + RD_RING) * RD_CTX_BYTES);
			DEV_ALLOC(e->d_rd_src, s.nctu);
		}
		if (e->cfg.bitrate_mode != 0 || s.rd_mode == RDM_FULL) {      // (RD_FULL: a step's estimates copy coder states the steps before must have produced)
			std::vector<uint16_t> need;
			if (!rc_need_table(s.wctu, s.hctu, s.sao, e->cfg.wfpp_num_threads > 1, need)) {
				hmr_set_error("hmr_gpu_enc_create: rate control: the reference's entropy-coding lag is not row-monotone on a %d x %d CTU grid", s.wctu, s.hctu);
				return HMR_GPU_ERR_ARG;
			}
			DEV_ALLOC(e->d_rc_need, need.size());
			HIP_TRY(hipMemcpy(e->d_rc_need, need.data(), need.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
		}
	}
	DEV_ALLOC(e->d_bytes, (size_t)s.width * s.height * 3 / 2);
	e->units_stride = s.wctu * 16;
	e->units_rows = s.hctu * 16;
	const size_t nu = (size_t)e->units_stride * e->units_rows;
	DEV_ALLOC(e->d_mvx, nu); DEV_ALLOC(e->d_mvy, nu); DEV_ALLOC(e->d_ref, nu); DEV_ALLOC(e->d_qp, nu);
	DEV_ALLOC(e->d_flags, nu);
	DEV_ALLOC(e->d_public, sizeof(CtuPublic) * s.nctu);
	e->h_public.resize(sizeof(CtuPublic) * s.nctu);
	e->h_coeff.resize((size_t)6144 * s.nctu);
	e->d.seq = e->d_seq;
	e->d.frame = e->d_frame;
	e->d.tables = ctx->tables;
	e->d.geo = e->d_geo;
	e->d.rc_dyn = e->d_rc_dyn;
	{
		const size_t oy = (size_t)s.margin_y * s.stride_y + s.margin_y, oc = (size_t)s.margin_c * s.stride_c + s.margin_c;
		PostPic &P = e->d.post;
		memset(&P, 0, sizeof P);
		P.dbk[0] = e->d_pre[0] + oy; P.dbk[1] = e->d_pre[1] + oc; P.dbk[2] = e->d_pre[2] + oc;
		P.units_stride = e->units_stride;
		P.mvx = e->d_mvx; P.mvy = e->d_mvy; P.ref = e->d_ref; P.uqp = e->d_qp; P.flags = e->d_flags;
		P.rows = e->d_rows; P.ent = e->d_ent; P.bs = e->d_bs; P.row_cap = e->row_cap; P.cumbits = e->d_cumbits;
		P.sao_lambda = e->d_sao_tab; P.errors = e->d_post_err; P.rc_need = e->d_rc_need;
		P.prof = (unsigned long long *)(e->d_post_err + 4);      // (profiling build)
		e->d.fin = (double *)(e->d_post_err + 4 + 2 * 16);
	}
	e->cur = 0;
	e->d.raster = e->raster;
	e->d.threads = e->cfg.wfpp_num_threads > 1 ? e->cfg.wfpp_num_threads : 1;
	e->last_ms = e->last_total_ms = 0;
	e->last_passes = e->last_encodes = 0;
	HIP_TRY(hipStreamSynchronize(ctx->stream));   // (the buffers are cleared by now)
	guard.ok = true;
	*out = e;
	return HMR_GPU_OK;
}

extern "C" int hmr_gpu_enc_create(hmr_gpu_ctx *ctx, const hmr_gpu_enc_cfg *cfg, hmr_gpu_enc **out) { return enc_create(ctx, cfg, -1, out); }
// wfpp_num_threads = 1 for BATCHES: the reference's deterministic single-thread order, CTU by CTU in raster order, as tasks of the pool (EncDev::raster) - one decision in
// flight per picture, so it is many pictures per launch that fill the device.  (hmr_gpu_enc_create runs a fixed-QP, RD_FAST encoder with one thread through the
// cooperative guess / verify / re-encode schedule, which is the faster way for ONE sequence and is not a batch schedule.)
extern "C" int hmr_gpu_enc_create_serial_pool(hmr_gpu_ctx *ctx, const hmr_gpu_enc_cfg *cfg, hmr_gpu_enc **out)
{
	if (!cfg || cfg->wfpp_num_threads > 1 || cfg->num_enc_engines > 1) {
		hmr_set_error("hmr_gpu_enc_create_serial_pool: wfpp_num_threads and num_enc_engines must be 1");
		return HMR_GPU_ERR_ARG;
	}
	g_serial_pool = 1;
	const int rc = enc_create(ctx, cfg, -1, out);
	g_serial_pool = 0;
	return rc;
}
extern "C" int hmr_gpu_enc_create_engine(hmr_gpu_ctx *ctx, const hmr_gpu_enc_cfg *cfg, int engine_index, hmr_gpu_enc **out)
{
	if (engine_index < 0) return HMR_GPU_ERR_ARG;
	return enc_create(ctx, cfg, engine_index, out);
}
// A second object for the SAME engine: it shares the engine's persistent state (the CTU records and the WPP threads' mode buffers, which a frame continues from the
// engine's previous frame) with `of` and has pictures, filter state and sub-stream buffers of its own - so that hmr_gpu_enc_encode_chain can hold the engine's next frame
// in the same launch (it starts when the one before it is finished, as the reference's engine does).  Destroy the twins before the object they were made from.
extern "C" int hmr_gpu_enc_create_engine_twin(hmr_gpu_ctx *ctx, hmr_gpu_enc *of, hmr_gpu_enc **out)
{
	if (!ctx || !of || !out || of->engine_index < 0 || of->twin_of) return HMR_GPU_ERR_ARG;
	hmr_gpu_enc *t = nullptr;
	const int rc = enc_create(ctx, (const hmr_gpu_enc_cfg *)&of->cfg, of->engine_index, &t);
	if (rc) return rc;
	(void)hipFree(t->d_ctus_eng[0]);
	(void)hipFree(t->d_rowstate_eng[0]);
	(void)hipFree(t->d_seen_eng[0]);
	t->d_ctus_eng[0] = of->d_ctus_eng[0];
	t->d_rowstate_eng[0] = of->d_rowstate_eng[0];
	t->d_seen_eng[0] = of->d_seen_eng[0];
	t->d.ctus = t->d_ctus_eng[0]; t->d.rowstate = t->d_rowstate_eng[0]; t->d.thread_seen = t->d_seen_eng[0];
	t->twin_of = of;
	*out = t;
	return HMR_GPU_OK;
}
extern "C" int hmr_gpu_enc_state_bytes(void) { return (int)sizeof(HostState); }
extern "C" long hmr_gpu_enc_reference_elems(hmr_gpu_enc *e, int comp) { return e && comp >= 0 && comp < 3 ? (long)e->pic_elems[comp] : -1; }

// The picture the next frame predicts from (padded planes, from the first element of their allocation) and the frame-to-frame scalars: what one engine hands
// to the next (encoder_engine_thread keeps both in the shared hvenc_enc_t; with an engine per GPU they travel).  Device buffers of hmr_gpu_enc_reference_elems.
extern "C" int hmr_gpu_enc_export_reference(hmr_gpu_enc *e, int16_t *dy, int16_t *du, int16_t *dv, void *state)
{
	if (!e || !dy || !du || !dv || !state) return HMR_GPU_ERR_ARG;
	hipStream_t st = e->ctx->stream;
	HIP_TRY(hipSetDevice(e->ctx->device));
	int16_t *dst[3] = {dy, du, dv};
	for (int c = 0; c < 3; c++) HIP_TRY(hipMemcpyAsync(dst[c], e->d_pic[e->cur][c], e->pic_elems[c] * 2, hipMemcpyDeviceToDevice, st));
	HIP_TRY(hipStreamSynchronize(st));
	memcpy(state, &e->st, sizeof(HostState));
	return HMR_GPU_OK;
}
extern "C" int hmr_gpu_enc_import_reference(hmr_gpu_enc *e, const int16_t *dy, const int16_t *du, const int16_t *dv, const void *state)
{
	if (!e || !dy || !du || !dv || !state) return HMR_GPU_ERR_ARG;
	HostState in;
	memcpy(&in, state, sizeof in);
	if (in.engines != e->st.engines || (e->engine_index >= 0 && in.num_encoded_frames % e->st.engines != e->engine_index)) {
		hmr_set_error("hmr_gpu_enc_import_reference: state of frame %d does not precede a frame of engine %d of %d", in.num_encoded_frames - 1, e->engine_index, e->st.engines);
		return HMR_GPU_ERR_ARG;
	}
	hipStream_t st = e->ctx->stream;
	HIP_TRY(hipSetDevice(e->ctx->device));
	const int16_t *src[3] = {dy, du, dv};
	for (int c = 0; c < 3; c++) HIP_TRY(hipMemcpyAsync(e->d_pic[e->cur][c], src[c], e->pic_elems[c] * 2, hipMemcpyDeviceToDevice, st));
	HIP_TRY(hipStreamSynchronize(st));
	e->st = in;
	return HMR_GPU_OK;
}

// The same hand-over for the engines of a step at once, with the picture as it travels between GPUs: 8-bit samples without margins (width x height luma, then the
// two width / 2 x height / 2 chroma planes: hmr_gpu_enc_reference_bytes), picture i at dev_rows + i * pitch; the importer widens it and pads the margins
// (reference_picture_border_padding_ctu: the margins are a function of the picture).  states: n x hmr_gpu_enc_state_bytes() bytes of host memory.
extern "C" long hmr_gpu_enc_reference_bytes(hmr_gpu_enc *e) { return e ? (long)e->seq.width * e->seq.height * 3 / 2 : -1; }
extern "C" int hmr_gpu_enc_export_references8(hmr_gpu_enc **encs, int n, uint8_t *dev_rows, long pitch, void *states)
{
	if (!encs || n <= 0 || !dev_rows || !states) return HMR_GPU_ERR_ARG;
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		if (!e || pitch < hmr_gpu_enc_reference_bytes(e)) return HMR_GPU_ERR_ARG;
		HIP_TRY(hipSetDevice(e->ctx->device));
		const int rc = narrow_packed(e, dev_rows + (size_t)i * pitch);
		if (rc) return rc;
		memcpy((uint8_t *)states + (size_t)i * sizeof(HostState), &e->st, sizeof(HostState));
	}
	for (int i = 0; i < n; i++) HIP_TRY(hipStreamSynchronize(encs[i]->ctx->stream));
	return HMR_GPU_OK;
}
extern "C" int hmr_gpu_enc_import_references8(hmr_gpu_enc **encs, int n, const uint8_t *dev_rows, long pitch, const void *states)
{
	if (!encs || n <= 0 || !dev_rows || !states) return HMR_GPU_ERR_ARG;
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		if (!e || pitch < hmr_gpu_enc_reference_bytes(e)) return HMR_GPU_ERR_ARG;
		HostState in;
		memcpy(&in, (const uint8_t *)states + (size_t)i * sizeof(HostState), sizeof in);
		if (in.engines != e->st.engines || (e->engine_index >= 0 && in.num_encoded_frames % e->st.engines != e->engine_index)) {
			hmr_set_error("hmr_gpu_enc_import_references8: engine %d: state of frame %d does not precede a frame of engine %d of %d", i, in.num_encoded_frames - 1, e->engine_index, e->st.engines);
			return HMR_GPU_ERR_ARG;
		}
		const Seq &s = e->seq;
		HIP_TRY(hipSetDevice(e->ctx->device));
		int16_t *dst[3] = {plane0(e, e->cur, 0), plane0(e, e->cur, 1), plane0(e, e->cur, 2)};
		int rc = widen_packed(e, dev_rows + (size_t)i * pitch, dst, s.stride_y, s.stride_c);
		if (rc) return rc;
		hmr_gpu_frame fr = {s.width, s.height, dst[0], dst[1], dst[2], s.stride_y, s.stride_c};
		rc = hmr_gpu_pad_frame(e->ctx, &fr, s.margin_y, s.margin_y);
		if (rc) return rc;
		e->st = in;
	}
	for (int i = 0; i < n; i++) HIP_TRY(hipStreamSynchronize(encs[i]->ctx->stream));
	return HMR_GPU_OK;
}

extern "C" void hmr_gpu_enc_destroy(hmr_gpu_enc *e)
{
	if (!e) return;
	(void)hipSetDevice(e->ctx->device);
	(void)hipStreamSynchronize(e->ctx->stream);
	release_planes(e);
	for (PlaneSet *ps : {&e->chain_planes, &e->chain_planes2})
		if (ps->y) { (void)hipFree(ps->y); (void)hipFree(ps->c[0]); (void)hipFree(ps->c[1]); }
	e->d.ctus = e->d_ctus_eng[0]; e->d.rowstate = e->d_rowstate_eng[0]; e->d.thread_seen = e->d_seen_eng[0];
	if (e->twin_of) e->d.ctus = nullptr, e->d.rowstate = nullptr, e->d.thread_seen = nullptr;      // (they belong to the object the twin was made from)
	for (int k = 1; k < MAX_ENGINES; k++) {
		if (e->d_ctus_eng[k]) (void)hipFree(e->d_ctus_eng[k]);
		if (e->d_rowstate_eng[k]) (void)hipFree(e->d_rowstate_eng[k]);
		if (e->d_seen_eng[k]) (void)hipFree(e->d_seen_eng[k]);
	}
	if (e->ev_frame) (void)hipEventDestroy(e->ev_frame);
	if (e->ev_ready) (void)hipEventDestroy(e->ev_ready);
	if (e->ev_batch0) (void)hipEventDestroy(e->ev_batch0);
	if (e->ev_batch1) (void)hipEventDestroy(e->ev_batch1);
	if (e->ev_decided) (void)hipEventDestroy(e->ev_decided);
	if (e->d_frames) (void)hipFree(e->d_frames);
	if (e->h_frames) (void)hipHostFree(e->h_frames);
	if (e->h_devs) (void)hipHostFree(e->h_devs);
	for (int k = 0; k < 2; k++) if (e->plane_stream[k]) { (void)hipStreamSynchronize(e->plane_stream[k]); (void)hipStreamDestroy(e->plane_stream[k]); }
	for (int k = 0; k < 3; k++) if (e->ev_plane[k]) (void)hipEventDestroy(e->ev_plane[k]);
	if (e->copy_stream) { (void)hipStreamSynchronize(e->copy_stream); (void)hipStreamDestroy(e->copy_stream); }
	if (e->d_gather) (void)hipFree(e->d_gather);
	if (e->h_gather) (void)hipHostFree(e->h_gather);
	if (e->h_offs) (void)hipHostFree(e->h_offs);
	e->rings.release();
	if (e->ev_pic_done) (void)hipEventDestroy(e->ev_pic_done);
	if (e->ev_own_done) (void)hipEventDestroy(e->ev_own_done);
	if (e->d_batch) (void)hipFree(e->d_batch);
	if (e->d_pool_state) (void)hipFree(e->d_pool_state);
	if (e->d_pool_slow) (void)hipFree(e->d_pool_slow);
	if (e->d_stage) (void)hipFree(e->d_stage);
	if (e->h_stage) (void)hipHostFree(e->h_stage);
	void *p[] = {e->d_seq, e->d_frame, e->d_geo, e->d.ctus, e->d.ctus_start, e->d.work_slow, e->d.coeff, e->d.progress, e->d.prefix, e->d.prof, e->d.guess, e->d.truth, e->d.outtok,
		     e->d.chain_start, e->d.chain_end, e->d.valid, e->d.dirty, e->d.hash, e->d.intra_before, e->d.used_intra, e->d.used_parts, e->d.counters, e->d.rowstate, e->d.thread_seen, e->d.row0_checked, e->d_bytes, e->d_mvx,
		     e->d_mvy, e->d_ref, e->d_qp, e->d_flags, e->d_public};
	for (void *q : p) (void)hipFree(q);
	for (int c = 0; c < 3; c++) {
		(void)hipFree(e->d_pic[0][c]);
		(void)hipFree(e->d_pic[1][c]);
		(void)hipFree(e->d_pre[c]);
		(void)hipFree(e->d_rec[c]);
	}
	{
		void *pp[] = {e->d_rows, e->d_ent, e->d_bs, e->d_cumbits, e->d_sao_tab, e->d_post_err, e->d_rc_need, e->d_rc_dyn, e->d_ctx_ring, e->d_rd_init, e->d_rd_src};
		for (void *q : pp) (void)hipFree(q);
	}
	for (auto &sl : e->src)
		for (int c = 0; c < 3; c++) (void)hipFree(sl.p[c]);
	delete e;
	g_plane_pool.encoder_destroyed();
}

// profiling build (-DHENC_POST_PROFILE): s_memtime ticks per part of the post-decision stage since the encoder was created (enc_post.h PostProf), 16 entries
extern "C" int hmr_gpu_enc_post_profile(hmr_gpu_enc *e, unsigned long long *out)
{
	if (!e || !out) return HMR_GPU_ERR_ARG;
	HIP_TRY(hipMemcpy(out, e->d_post_err + 4, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
#if defined(HENC_POST_PROFILE)
	HIP_TRY(hipMemcpyFromSymbol(out + 10, HIP_SYMBOL(g_ent_prof), 6 * sizeof(unsigned long long)));
#endif
	return HMR_GPU_OK;
}

extern "C" float hmr_gpu_enc_last_ctu_ms(hmr_gpu_enc *e) { return e ? e->last_ms : 0.f; }

extern "C" int hmr_gpu_enc_stale_predictions(hmr_gpu_enc *e, long *last_picture, long *all_pictures)
{
	if (!e) return HMR_GPU_ERR_ARG;
	if (last_picture) *last_picture = e->stale_last;
	if (all_pictures) *all_pictures = e->stale_total;
	return HMR_GPU_OK;
}

extern "C" int hmr_gpu_enc_last_stats(hmr_gpu_enc *e, int *passes, int *ctu_encodes, float *ctu_ms, float *frame_ms)
{
	if (!e) return HMR_GPU_ERR_ARG;
	if (passes) *passes = e->last_passes;
	if (ctu_encodes) *ctu_encodes = e->last_encodes;
	if (ctu_ms) *ctu_ms = e->last_ms;
	if (frame_ms) *frame_ms = e->last_total_ms;
	return HMR_GPU_OK;
}

extern "C" int hmr_gpu_enc_last_pool_kernel(hmr_gpu_enc *e) { return e ? e->last_pool_kernel : -1; }

// profiling build: per CTU, 100 MHz timestamps of {wait start, encode start, first use of the intra share (0: none), end} in the row-per-thread schedule
extern "C" int hmr_gpu_enc_timeline(hmr_gpu_enc *e, unsigned long long *out)
{
	if (!e || !out) return HMR_GPU_ERR_ARG;
	HIP_TRY(hipMemcpy(out, e->d.prof + (size_t)e->seq.hctu * PF_COUNT, sizeof(unsigned long long) * e->seq.nctu * 4, hipMemcpyDeviceToHost));
	return HMR_GPU_OK;
}

// profiling build (-DHENC_PROFILE): per-row phase timers in s_memtime ticks, [hctu][PF_COUNT]; all zero otherwise
extern "C" int hmr_gpu_enc_profile(hmr_gpu_enc *e, unsigned long long *out, int reset)
{
	if (!e || !out) return HMR_GPU_ERR_ARG;
	HIP_TRY(hipMemcpy(out, e->d.prof, sizeof(unsigned long long) * e->seq.hctu * PF_COUNT, hipMemcpyDeviceToHost));
	if (reset) {
		HIP_TRY(hipMemsetAsync(e->d.prof, 0, sizeof(unsigned long long) * e->seq.hctu * PF_COUNT, e->ctx->stream));
		HIP_TRY(hipStreamSynchronize(e->ctx->stream));
	}
	return HMR_GPU_OK;
}

extern "C" int hmr_gpu_enc_load_source(hmr_gpu_enc *e, int slot, const uint8_t *y, const uint8_t *u, const uint8_t *v)
{
	if (!e || slot < 0 || slot > 4096 || !y || !u || !v) return HMR_GPU_ERR_ARG;
	HIP_TRY(hipSetDevice(e->ctx->device));
	while ((int)e->src.size() <= slot) {
		SrcSlot sl;
		for (int c = 0; c < 3; c++) DEV_ALLOC(sl.p[c], e->src_elems[c]);
		e->src.push_back(sl);
	}
	return load_planes(e, y, u, v, e->src[slot].p, e->seq.src_stride_y, e->seq.src_stride_c);
}

extern "C" int hmr_gpu_enc_frame_ctus(hmr_gpu_enc *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, int image_type, const uint8_t *ref_y, const uint8_t *ref_u,
				      const uint8_t *ref_v, double avg_dist, uint8_t *records)
{
	if (!e || !y || !u || !v) return HMR_GPU_ERR_ARG;
	const Seq &s = e->seq;
	hipStream_t st = e->ctx->stream;
	HIP_TRY(hipSetDevice(e->ctx->device));
	int rc = hmr_gpu_enc_load_source(e, 0, y, u, v);
	if (rc) return rc;
	rc = set_frame(e, 0, image_type, avg_dist);
	if (rc) return rc;
	if (ref_y && ref_u && ref_v) {
		int16_t *dst[3] = {plane0(e, e->cur ^ 1, 0), plane0(e, e->cur ^ 1, 1), plane0(e, e->cur ^ 1, 2)};
		rc = load_planes(e, ref_y, ref_u, ref_v, dst, s.stride_y, s.stride_c);
		if (rc) return rc;
		hmr_gpu_frame fr = {s.width, s.height, dst[0], dst[1], dst[2], s.stride_y, s.stride_c};
		rc = hmr_gpu_pad_frame(e->ctx, &fr, s.margin_y, s.margin_y);
		if (rc) return rc;
	}
	rc = run_ctu_passes(e);
	if (rc) return rc;
	// frame statistics (encoder_engine_thread :3217-3238)
	rc = download_public(e);
	if (rc) return rc;
	HIP_TRY(hipStreamSynchronize(st));
	end_frame(s, e->st, e->f, frame_acc_dist(s, e->cfg.wfpp_num_threads, [&](int n) { return ((const CtuPublic *)(e->h_public.data() + sizeof(CtuPublic) * n))->distortion; }));
	if (records) {
		std::vector<int16_t> rec[3];
		std::vector<uint8_t> truth((size_t)s.nctu * MODE_STATE_BYTES), chain_end(MODE_STATE_BYTES);
		std::vector<uint32_t> node0(3 * s.nctu);
		HIP_TRY(hipMemcpy(e->h_coeff.data(), e->d.coeff, e->h_coeff.size() * 2, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(truth.data(), e->d.truth, truth.size(), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(chain_end.data(), e->d.chain_end, MODE_STATE_BYTES, hipMemcpyDeviceToHost));
		for (int n = 0; n < s.nctu; n++) {
			Node nd;
			HIP_TRY(hipMemcpy(&nd, &e->d.ctus[n].nodes[0], sizeof(Node), hipMemcpyDeviceToHost));
			node0[3 * n] = nd.cost; node0[3 * n + 1] = nd.distortion; node0[3 * n + 2] = nd.sum;
		}
		for (int c = 0; c < 3; c++) {
			rec[c].resize(e->pic_elems[c]);
			HIP_TRY(hipMemcpy(rec[c].data(), e->d_rec[c], e->pic_elems[c] * 2, hipMemcpyDeviceToHost));
		}
		memset(records, 0, (size_t)REC_BYTES * s.nctu);
		for (int n = 0; n < s.nctu; n++) {
			uint8_t *o = records + (size_t)n * REC_BYTES;
			const CtuPublic &ci = *(const CtuPublic *)(e->h_public.data() + sizeof(CtuPublic) * n);
			int32_t hdr[8] = {0x43545544, e->f.num_encoded_frames, n, e->f.slice_type, (int32_t)node0[3 * n], (int32_t)node0[3 * n + 1], (int32_t)node0[3 * n + 2],
					  e->f.scene_cut_ctu >= 0 && n >= e->f.scene_cut_ctu};
			memcpy(o, hdr, 32); o += 32;
			for (int k = 0; k < 3; k++) { memcpy(o, ci.cbf[k], 256); o += 256; }
			memcpy(o, ci.intra_mode[0], 256); o += 256;
			memcpy(o, ci.intra_mode[1], 256); o += 256;
			const uint8_t *arrs[9] = {ci.inter_mode, ci.tr_idx, ci.pred_depth, ci.part_size_type, ci.pred_mode, ci.skipped, ci.merge, ci.merge_idx, ci.qp};
			for (int k = 0; k < 9; k++) { memcpy(o, arrs[k], 256); o += 256; }
			memcpy(o, ci.mv_ref_idx, 256); o += 256;
			memcpy(o, ci.mv_diff_ref_idx, 256); o += 256;
			memcpy(o, ci.mv_ref, 2048); o += 2048;
			memcpy(o, ci.mv_diff, 2048); o += 2048;
			memcpy(o, e->h_coeff.data() + (size_t)n * 6144, 12288); o += 12288;
			// reconstruction before the loop filters: the part of the CTU inside the picture (the rest stays zero)
			for (int c = 0; c < 3; c++) {
				const int nn = c ? 32 : 64, px = (ci.x >> (c ? 1 : 0)), py = (ci.y >> (c ? 1 : 0));
				const int pw = c ? s.width / 2 : s.width, ph = c ? s.height / 2 : s.height, rs = c ? s.stride_c : s.stride_y, m = c ? s.margin_c : s.margin_y;
				const int16_t *p = rec[c].data() + (size_t)m * rs + m;
				for (int yy = 0; yy < nn; yy++) {
					if (py + yy < ph) {
						const int ww = px + nn <= pw ? nn : pw - px;
						memcpy(o, p + (size_t)(py + yy) * rs + px, ww * 2);
					}
					o += nn * 2;
				}
			}
			// the single thread's mode buffers after the CTU
			memcpy(o, n + 1 < s.nctu ? truth.data() + (size_t)(n + 1) * MODE_STATE_BYTES : chain_end.data(), MODE_STATE_BYTES);
		}
	}
	return e->f.slice_type;
}

namespace {
constexpr int CHAIN_MAX_FRAMES = 32;    // frames of one hmr_gpu_enc_encode_chain call
// A picture's gather record - what the host's bookkeeping needs of a picture of a pool launch, in one small download: a GatherHead, the CTUs' distortions (a word
// each: gather_dist), a gap, and in its last POST_MAX_ROWS words the bytes of the rows' sub-streams (gather_row_bytes).  Record i of a launch starts at word
// i * gather_pitch(the largest CTU count among the launch's pictures).  The buffers are declared as words - the distortions and byte counts are words - and a
// record's head is read and written through a GatherHead reference: the device and the host agree on the layout (one struct, one translation unit), the buffers come
// from hipMalloc / hipHostMalloc and nothing else aliases them.
constexpr int GATHER_HEAD = 12;         // words in front of the CTUs' distortions
struct GatherHead {
	int32_t failed_checks, encodes, scene_cut_ctu;      // EncDev::counters - the single-thread order's failed checks (the pool leaves 0), CTU encodes, the CTU that found a scene cut (-1: none)
	uint32_t flags;                                      // GATHER_*
	uint32_t sum_qp, bits;                               // rate control: the sum of the CTUs' QPs (the root nodes': acc_qp, hmr_encoder_lib.c:2938), the bits of all CTUs,
	double target_pict_size;                             // the picture target as the frame left it
	double launch_dist, avg_dist;                        // chains: the distortion total as the launch computed it, the average distortion the picture started from (the launch sets it for an engine's later pictures)
};
static_assert(sizeof(GatherHead) == GATHER_HEAD * 4, "the record's head is GATHER_HEAD words");
// flags: a row's sub-stream outgrew its buffer; the launch was abandoned by its watchdog; from bit 8 the picture's evaluations on a stale prediction window (Q12), saturating
constexpr uint32_t GATHER_ROW_OVERFLOW = 1u << 0, GATHER_ABANDONED = 1u << 1, GATHER_STALE_MAX = 0xffffffu;
constexpr int GATHER_STALE_SHIFT = 8;
// An EVEN number of words: the buffers start on 256 bytes, so every record - and with it the doubles of its head - starts on 8 bytes and the members are stored and
// read as they are (an odd pitch would need byte-wise access: a double stored through a misaligned pointer faults on the device).  The buffers are the encoder's own.
__host__ __device__ constexpr int gather_pitch(int max_nctu) { return (GATHER_HEAD + max_nctu + POST_MAX_ROWS + 1) & ~1; }
template <class W> __host__ __device__ W *gather_dist(W *rec) { return rec + GATHER_HEAD; }
template <class W> __host__ __device__ W *gather_row_bytes(W *rec, int pitch) { return rec + pitch - POST_MAX_ROWS; }

__global__ void k_gather_results(const EncDev *devs, uint32_t *out, int pitch, const int *pool_flags)
{
	const EncDev &d = devs[blockIdx.x];
	uint32_t *o = out + (size_t)blockIdx.x * pitch;
	GatherHead &h = *(GatherHead *)o;
	const int nctu = d.seq->nctu;
	__shared__ uint32_t s_qp, s_bits, s_stale;
	if (threadIdx.x == 0) { s_qp = 0; s_bits = 0; s_stale = 0; }
	__syncthreads();
	uint32_t q = 0, b = 0, stale = 0;
	for (int c = threadIdx.x; c < nctu; c += blockDim.x) { q += d.ctus[c].nodes[0].qp; stale += (uint32_t)d.ctus[c].n_stale_pred; }
	for (int r = threadIdx.x; r < d.seq->hctu; r += blockDim.x) b += d.post.cumbits[r * d.seq->wctu + d.seq->wctu - 1];
	atomicAdd(&s_qp, q);
	atomicAdd(&s_bits, b);
	atomicAdd(&s_stale, stale);
	__syncthreads();
	if (threadIdx.x == 0) {
		h.failed_checks = d.counters[0]; h.encodes = d.counters[1]; h.scene_cut_ctu = d.counters[2];
		h.flags = (d.post.errors[0] != 0 ? GATHER_ROW_OVERFLOW : 0) | (pool_flags && pool_flags[1] != 0 ? GATHER_ABANDONED : 0) | ((s_stale > GATHER_STALE_MAX ? GATHER_STALE_MAX : s_stale) << GATHER_STALE_SHIFT);
		h.sum_qp = s_qp;
		h.bits = s_bits;
		h.target_pict_size = d.counters[2] >= 0 ? d.rc_dyn->target_pict_size : d.frame->rc.target_pict_size;
		h.launch_dist = d.fin[0];
		h.avg_dist = d.frame->avg_dist;
	}
	for (int c = threadIdx.x; c < nctu; c += blockDim.x) gather_dist(o)[c] = d.ctus[c].distortion;
	for (int r = threadIdx.x; r < d.seq->hctu; r += blockDim.x) gather_row_bytes(o, pitch)[r] = (uint32_t)d.post.ent[r].bytecnt;
}

// a device buffer and its page-locked twin on the host, grown to `want` elements when they hold fewer than `need`
template <class T>
int grow_pair(T **dev, T **host, size_t *have, size_t need, size_t want)
{
	if (need <= *have) return HMR_GPU_OK;
	if (*dev) (void)hipFree(*dev);
	if (*host) (void)hipHostFree(*host);
	*dev = *host = nullptr;
	*have = 0;
	HIP_TRY(hipMalloc((void **)dev, want * sizeof(T)));
	HIP_TRY(hipHostMalloc((void **)host, want * sizeof(T), hipHostMallocDefault));
	*have = want;
	return HMR_GPU_OK;
}
// What the lead of a pool launch of n pictures of up to max_nctu CTUs owns: the device copies of their EncDev records, room for `records` gather records and - where
// the pictures are staged through k_batch_stage (records = BATCH_MAX; one picture on its own uploads its record and parameters itself) - the staging arrays.
int launch_buffers(hmr_gpu_enc *lead, int n, int max_nctu, int records)
{
	const int pitch = lead->record_words = gather_pitch(max_nctu);
	if (records > 1 && !lead->d_frames) {
		HIP_TRY(hipMalloc((void **)&lead->d_frames, BATCH_MAX * sizeof(FrameCtx)));
		HIP_TRY(hipHostMalloc((void **)&lead->h_frames, BATCH_MAX * sizeof(FrameCtx), hipHostMallocDefault));
		HIP_TRY(hipHostMalloc((void **)&lead->h_devs, BATCH_MAX * sizeof(EncDev), hipHostMallocDefault));
	}
	if (!lead->d_batch) HIP_TRY(hipMalloc((void **)&lead->d_batch, BATCH_MAX * sizeof(EncDev)));
	return grow_pair(&lead->d_gather, &lead->h_gather, &lead->gather_words, (size_t)pitch * n, (size_t)pitch * records);
}
// behind a pool launch of n pictures on the lead's stream: their gather records, and the records' download
int queue_gather(hmr_gpu_enc *lead, int n)
{
	hipStream_t st = lead->ctx->stream;
	const int pitch = lead->record_words;
	hipLaunchKernelGGL(k_gather_results, dim3(n), dim3(256), 0, st, (const EncDev *)lead->d_batch, lead->d_gather, pitch, (const int *)(lead->d_pool_state + BATCH_MAX * POOL_STRIDE));
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(lead->h_gather, lead->d_gather, (size_t)pitch * n * 4, hipMemcpyDeviceToHost, st));
	return HMR_GPU_OK;
}

// The downloaded record of picture `index` of lead's launch, e's picture, read for a call of `entry` ("<the entry's name>: <its word for a picture>", for the
// messages): refuses a launch its watchdog abandoned and a sub-stream that outgrew its buffer, notes the launch's counters in e and hands back what the frame's
// bookkeeping needs (dist: the CTUs' distortions; row_bytes: the bytes of the rows' sub-streams).
struct PictureResults { FrameRcOut rc; double launch_dist, avg_dist; const uint32_t *dist, *row_bytes; };
int read_record(hmr_gpu_enc *lead, int index, hmr_gpu_enc *e, const char *entry, PictureResults *out)
{
	const uint32_t *rec = lead->h_gather + (size_t)index * lead->record_words;
	const GatherHead &h = *(const GatherHead *)rec;
	if (h.flags & GATHER_ABANDONED) {
		hmr_set_error("k_encode_pool: the launch was abandoned by its watchdog (a worker found nothing to do for too long: HENC_WATCHDOG_S)");
		return HMR_GPU_ERR_HIP;
	}
	if (h.flags & GATHER_ROW_OVERFLOW) {
		hmr_set_error("%s %d: a CTU row's sub-stream outgrew its buffer (%d bytes)", entry, index, e->row_cap);
		return HMR_GPU_ERR_HIP;
	}
	e->note_stale_predictions(h.flags >> GATHER_STALE_SHIFT);
	e->last_encodes = h.encodes;
	e->f.scene_cut_ctu = h.scene_cut_ctu;
	e->last_passes = 1;
	out->rc.sum_qp = (int)h.sum_qp; out->rc.consumed_bits = (double)h.bits; out->rc.target_pict_size = h.target_pict_size;
	out->launch_dist = h.launch_dist; out->avg_dist = h.avg_dist;
	out->dist = gather_dist(rec);
	out->row_bytes = gather_row_bytes(rec, lead->record_words);
	return HMR_GPU_OK;
}

// One picture in the row-per-thread schedule (hmr_gpu_enc_encode_source): it is its own lead.  LAUNCH - its EncDev record and parameters go up by copies of their
// own, not through k_batch_stage: a lone sequence's launches per frame stay what they are ...
int lockstep_launch(hmr_gpu_enc *e)
{
	const Seq &s = e->seq;
	hipStream_t st = e->ctx->stream;
	int rc = ctu_stage_prepare(e);
	if (rc) return rc;
	HIP_TRY(hipEventRecord(e->ctx->ev0, st));
	if ((rc = launch_buffers(e, 1, s.nctu, 1))) return rc;
	HIP_TRY(hipMemcpyAsync(e->d_batch, &e->d, sizeof(EncDev), hipMemcpyHostToDevice, st));
	if ((rc = launch_pool(e, &e->d, 1, e->raster ? pool_inflight(s, 1) : s.hctu, s.rd_mode == RDM_FULL, st))) return rc;      // (one picture: a worker per row, each on a CU of its own)
	HIP_TRY(hipEventRecord(e->ctx->ev1, st));
	return HMR_GPU_OK;
}
// ... and COLLECT, once queue_gather's download has been waited for: the CTU stage is over (entry: read_record's)
int lockstep_collect(hmr_gpu_enc *e, const char *entry, PictureResults *res)
{
	release_planes(e);
	HIP_TRY(hipEventElapsedTime(&e->last_ms, e->ctx->ev0, e->ctx->ev1));
	return read_record(e, 0, e, entry, res);
}
// run_ctu_passes, that is hmr_gpu_enc_frame_ctus on a row-per-thread object: the CTU stage from start to end.  Its collect is the record too (the parent fetched the
// counters and the abandoned flag by two copies of their own), so this entry also counts the stale predictions and refuses a sub-stream that outgrew its buffer.
int lockstep_run(hmr_gpu_enc *e)
{
	PictureResults res;
	int rc = lockstep_launch(e);
	if (rc || (rc = queue_gather(e, 1))) return rc;
	HIP_TRY(hipStreamSynchronize(e->ctx->stream));
	return lockstep_collect(e, "hmr_gpu_enc_frame_ctus: picture", &res);
}

// a picture's sub-streams, as many bytes as each row took, one after the other into e->h_bs: a copy per row queued on `st` (frame_assemble reads them once it has been waited for)
int queue_substreams(hmr_gpu_enc *e, const uint32_t *row_bytes, hipStream_t st)
{
	const int rows = e->seq.wpp ? e->seq.hctu : 1;
	size_t total = 0;
	for (int r = 0; r < rows; r++) total += row_bytes[r];
	if (e->h_bs.size() < total) e->h_bs.resize(total);      // (the host copy holds what the picture took, not the rows' whole buffers)
	total = 0;
	for (int r = 0; r < rows; r++) {
		HIP_TRY(hipMemcpyAsync(e->h_bs.data() + total, e->d_bs + (size_t)r * e->row_cap, row_bytes[r], hipMemcpyDeviceToHost, st));
		total += row_bytes[r];
	}
	return HMR_GPU_OK;
}

}  // namespace

// HOMER_enc_encode for one picture already on the device (hmr_gpu_enc_load_source): CTU decisions, deblocking, SAO, entropy coding of the CTU rows' sub-streams and
// border padding on the device (the CTU kernel and its post-decision tasks, enc_post.h); the host writes the headers and assembles the access unit.
namespace {
// the access unit of frame `f` from the rows' sub-streams (`bytes`: the sub-streams one after the other) into `stream`
int frame_assemble(hmr_gpu_enc *e, const FrameCtx &f, const uint8_t *bytes, const uint32_t *row_bytes, uint8_t *stream, long cap, long *stream_bytes)
{
	const Seq &s = e->seq;
	const int rows = s.wpp ? s.hctu : 1;
	std::vector<const uint8_t *> data(rows);
	std::vector<int> nb(rows);
	size_t o = 0;
	for (int r = 0; r < rows; r++) { data[r] = bytes + o; nb[r] = (int)row_bytes[r]; o += row_bytes[r]; }
	std::vector<uint8_t> out;
	assemble_access_unit(e->es, s, f, e->cfg.profile, data.data(), nb.data(), out);
	*stream_bytes = (long)out.size();
	if ((long)out.size() > cap) {
		hmr_set_error("hmr_gpu_enc_encode: the access unit needs %ld bytes, the buffer holds %ld", (long)out.size(), cap);
		return HMR_GPU_ERR_ARG;
	}
	memcpy(stream, out.data(), out.size());
	return f.slice_type;
}
// one sequence, behind its CTU stage (row-per-thread schedule: launched, and waited for here; single-thread order: over): the sub-streams and the CTUs' distortions
// to the host, the access unit, the frame bookkeeping
int frame_finish(hmr_gpu_enc *e, uint8_t *stream, long cap, long *stream_bytes, uint8_t *recon)
{
	const Seq &s = e->seq;
	hipStream_t st = e->ctx->stream;
	int rc, err[4];
	HIP_TRY(hipMemcpyAsync(e->h_ent.data(), e->d_ent, sizeof(RowEnt) * s.hctu, hipMemcpyDeviceToHost, st));
	if ((rc = e->lockstep ? queue_gather(e, 1) : download_public(e))) return rc;
	HIP_TRY(hipMemcpyAsync(err, e->d_post_err, sizeof err, hipMemcpyDeviceToHost, st));      // (err[3]: download_public's count)
	HIP_TRY(hipStreamSynchronize(st));
	PictureResults res;
	if (e->lockstep && (rc = lockstep_collect(e, "hmr_gpu_enc_encode: picture", &res))) return rc;      // (refuses an abandoned launch and a row overflow itself)
	if (getenv("HENC_DEBUG_POST")) {
		std::vector<PostRow> rows(s.hctu);
		HIP_TRY(hipMemcpy(rows.data(), e->d_rows, sizeof(PostRow) * s.hctu, hipMemcpyDeviceToHost));
		for (int r = 0; r < s.hctu; r++)
			fprintf(stderr, "post row %d: dec %d D %d/%d P %d/%d F %d/%d\n", r, rows[r].dec, rows[r].d_claim, rows[r].d_done, rows[r].p_claim, rows[r].p_done, rows[r].f_claim, rows[r].f_done);
		fprintf(stderr, "post errors %d %d %d %d, sao %d\n", err[0], err[1], err[2], err[3], s.sao);
	}
	if (err[0]) {      // (single-thread order only: on the row-per-thread path read_record has refused it above, and the rows' bytes come from the record, not from h_ent)
		hmr_set_error("hmr_gpu_enc_encode: a CTU row's sub-stream outgrew its buffer (%d bytes)", e->row_cap);
		return HMR_GPU_ERR_HIP;
	}
	if (err[2]) {
		hmr_set_error("hmr_gpu_enc_encode: the post-decision stage was abandoned by its watchdog");
		return HMR_GPU_ERR_HIP;
	}
	std::vector<uint32_t> ent_bytes(s.hctu);      // (single-thread order: the rows' bytes from their coders' records)
	for (int r = 0; r < s.hctu; r++) ent_bytes[r] = (uint32_t)e->h_ent[r].bytecnt;
	const uint32_t *row_bytes = e->lockstep ? res.row_bytes : ent_bytes.data();
	if ((rc = queue_substreams(e, row_bytes, st))) return rc;
	if (recon) {      // (the device path - k_egress into the staging buffer - plus one copy)
		if ((rc = narrow_packed(e, e->d_bytes))) return rc;
		HIP_TRY(hipMemcpyAsync(recon, e->d_bytes, (size_t)s.width * s.height * 3 / 2, hipMemcpyDeviceToHost, st));
	}
	HIP_TRY(hipStreamSynchronize(st));
	FrameRcOut ro = {0, 0.0, 0.0};
	if (e->lockstep) ro = res.rc;
	else e->note_stale_predictions((uint32_t)err[3]);
	const double acc = e->lockstep ? frame_acc_dist(s, e->cfg.wfpp_num_threads, [&](int n) { return res.dist[n]; })
				       : frame_acc_dist(s, e->cfg.wfpp_num_threads, [&](int n) { return ((const CtuPublic *)(e->h_public.data() + sizeof(CtuPublic) * n))->distortion; });
	// (a buffer that is too small loses the access unit; the sequence state has not moved on, but the device pictures have: the caller has to start over)
	rc = frame_assemble(e, e->f, e->h_bs.data(), row_bytes, stream, cap, stream_bytes);
	if (rc < 0) return rc;
	end_frame(s, e->st, e->f, acc, &ro);
	HIP_TRY(hipEventRecord(e->ctx->ev1, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipEventElapsedTime(&e->last_total_ms, e->ev_frame, e->ctx->ev1));
	return e->f.slice_type;
}
}  // namespace

extern "C" int hmr_gpu_enc_encode_source(hmr_gpu_enc *e, int slot, int image_type, uint8_t *stream, long cap, long *stream_bytes, uint8_t *recon)
{
	if (!e || slot < 0 || slot >= (int)e->src.size() || !stream || !stream_bytes) return HMR_GPU_ERR_ARG;
	if (e->awaiting_delivery) {
		hmr_set_error("hmr_gpu_enc_encode_source: the encoder has an access unit outstanding from a pipelined batch call: flush first");
		return HMR_GPU_ERR_ARG;
	}
	hipStream_t st = e->ctx->stream;
	HIP_TRY(hipSetDevice(e->ctx->device));
	HIP_TRY(hipEventRecord(e->ev_frame, st));
	int rc = set_frame(e, slot, image_type, -1.0);
	if (rc) return rc;
	rc = e->lockstep ? lockstep_launch(e) : run_ctu_passes(e);
	if (rc) return rc;
	return frame_finish(e, stream, cap, stream_bytes, recon);
}
