// Host side of the frame encoder, part 2 (included by k_encode.hip): several pictures per launch - hmr_gpu_enc_encode_batch / _batch_pipelined (independent
// sequences), hmr_gpu_enc_encode_chain (overlapped frames of one sequence) - and hmr_gpu_enc_encode.
// Several sequences, one frame each, with ONE launch for all their CTU stages (k_encode_pool): encs[i] encodes its picture slots[i] into streams[i].
// All encoders must use the row-per-thread schedule and live on the same device; each finishes its frame (filters, SAO, records and levels into the staging buffer)
// on its own stream.  The streams are those hmr_gpu_enc_encode_source would have produced one by one.
//
// A step has three parts: LAUNCH (frame set-up, phase planes, the pool launch), FINISH (after the launch: the frames' counters and distortions in one small
// download, frame bookkeeping, a host thread per sequence queues its filter chain and packs its records and levels into the staging buffer, whose download to the
// host is queued behind them on a copy stream) and DELIVER (wait for that download, a host thread per sequence codes its access unit).  The plain call runs
// LAUNCH, FINISH, DELIVER; the pipelined call runs LAUNCH(k), DELIVER(k - 1), FINISH(k), so that the download and the entropy coding of a step run while the
// device is busy with the next step's CTU stage (nothing of step k reads what DELIVER(k - 1) reads: the staging buffers are written again only in FINISH(k)).
namespace {
// the sub-streams of the pictures of a launch, row after row, into the staging buffer (picture i at out + offs[i]): what the host downloads to assemble the access units
__global__ __launch_bounds__(256) void k_pack_streams(const EncDev *devs, uint8_t *out, const size_t *offs)
{
	__shared__ uint32_t start[POST_MAX_ROWS + 1];
	const EncDev &d = devs[blockIdx.x];
	const int rows = d.seq->wpp ? d.seq->hctu : 1;
	if (threadIdx.x == 0) {
		uint32_t o = 0;
		for (int r = 0; r < rows; r++) { start[r] = o; o += (uint32_t)d.post.ent[r].bytecnt; }
		start[rows] = o;
	}
	__syncthreads();
	uint8_t *dst = out + offs[blockIdx.x];
	for (int r = 0; r < rows; r++) {
		const uint8_t *src = d.post.bs + (size_t)r * d.post.row_cap;
		const uint32_t n = start[r + 1] - start[r];
		for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) dst[start[r] + i] = src[i];
	}
}

// The batch's pictures: their EncDev records and frame parameters come from page-locked host memory (read by the kernel itself: a host-to-device copy queued here
// waited behind the previous step's 2 GB download on the copy engines - rocprofv3 trace, 35 ms), and what ctu_stage_prepare does for one picture is done for all.
__global__ void k_batch_stage(const EncDev *h_devs, const FrameCtx *h_frames, EncDev *d_devs, FrameCtx *d_frames)
{
	const int i = blockIdx.x, t = threadIdx.x;
	for (int k = t; k < (int)(sizeof(EncDev) / 4); k += blockDim.x) ((uint32_t *)(d_devs + i))[k] = ((const uint32_t *)(h_devs + i))[k];
	for (int k = t; k < (int)(sizeof(FrameCtx) / 4); k += blockDim.x) ((uint32_t *)(d_frames + i))[k] = ((const uint32_t *)(h_frames + i))[k];
	const EncDev d = h_devs[i];
	const int H = d.seq->hctu, W = d.seq->wctu;
	if (t < 3) d.counters[t] = t == 2 ? -1 : 0;
	if (t == 3) *d.row0_checked = 0;
	if (t >= 4 && t < 8) d.post.errors[t - 4] = 0;
	for (int k = t; k < H * (int)(sizeof(PostRow) / 4); k += blockDim.x) ((int *)d.post.rows)[k] = 0;
	for (int k = t; k < H; k += blockDim.x) d.progress[k] = 0;
	for (int k = t; k < H * (W + 1); k += blockDim.x) d.prefix[k] = 0;
}

struct BatchTimes {
	std::chrono::steady_clock::time_point t[8];
	double ms(int a, int b) const { return std::chrono::duration<double, std::milli>(t[b] - t[a]).count(); }
};

// fn(i) for i in [0, n) on up to `threads` host threads (sequence i goes to thread i mod threads).  A thread per sequence cost more in thread start-up than the
// few dozen stream calls a sequence needs; a dozen threads keep the runtime's submission path busy just as well.
template <class F>
void parallel_for(int n, int threads, F fn)
{
	const int T = n < threads ? n : threads;
	std::vector<std::thread> th;
	for (int t = 0; t < T; t++)
		th.emplace_back([=]() {
			for (int i = t; i < n; i += T) fn(i);
		});
	for (auto &x : th) x.join();
}
constexpr int QUEUE_THREADS = 16;       // for queueing device work
constexpr int CODING_THREADS = 32;      // for the access units (headers, entry points, escaping: a few microseconds per kilobyte)

int batch_check(hmr_gpu_enc **encs, int n, const int *slots, uint8_t **streams, const long *caps, long *stream_bytes)
{
	if (!encs || n <= 0 || n > BATCH_MAX || !streams || !caps || !stream_bytes) return HMR_GPU_ERR_ARG;
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		if (!e || !e->lockstep || e->ctx->device != encs[0]->ctx->device || (slots && (slots[i] < 0 || slots[i] >= (int)e->src.size())) || !streams[i]) {
			hmr_set_error("hmr_gpu_enc_encode_batch: encoder %d: needs the row-per-thread schedule (wfpp_num_threads > 1), the batch's device and a loaded picture slot", i);
			return HMR_GPU_ERR_ARG;
		}
		for (int j = 0; j < i; j++)
			if (encs[j] == e) return HMR_GPU_ERR_ARG;
	}
	return HMR_GPU_OK;
}

// The n pictures staged in lead->h_devs / h_frames (launch_buffers) as ONE pool launch on the lead's stream, their gather records and the records' download behind
// it.  rows_total, needs_rd: launch_pool's.
int submit_staged(hmr_gpu_enc *lead, int n, int rows_total, bool needs_rd)
{
	hipStream_t bst = lead->ctx->stream;
	hipLaunchKernelGGL(k_batch_stage, dim3(n), dim3(256), 0, bst, (const EncDev *)lead->h_devs, (const FrameCtx *)lead->h_frames, (EncDev *)lead->d_batch, lead->d_frames);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(lead->ev_batch0, bst));
	const int rc = launch_pool(lead, lead->h_devs, n, rows_total, needs_rd, bst);
	if (rc) return rc;
	(void)hipEventRecord(lead->ev_batch1, bst);
	return queue_gather(lead, n);
}
// the lead's stream waited for: the launch is over (CTU decisions, filters and entropy coding of every picture) and its records are on the host; ms: the pool's time
int wait_for_launch(hmr_gpu_enc *lead, float *ms)
{
	const hipError_t waited = hipStreamSynchronize(lead->ctx->stream);
	if (waited != hipSuccess) {
		hmr_set_error("k_encode_pool: %s", hipGetErrorString(waited));
		return HMR_GPU_ERR_HIP;
	}
	HIP_TRY(hipEventElapsedTime(ms, lead->ev_batch0, lead->ev_batch1));
	return HMR_GPU_OK;
}

// LAUNCH: the frames' CTU stages as one pool launch on the lead encoder's stream, their counters and distortions gathered behind it
int batch_launch(hmr_gpu_enc **encs, int n, const int *slots, const int *image_types)
{
	hmr_gpu_enc *lead = encs[0];
	hipStream_t bst = lead->ctx->stream;
	int rc, rows_total = 0, max_ctus = 0;
	bool needs_rd = false;
	for (int i = 0; i < n; i++)
		if (encs[i]->seq.nctu > max_ctus) max_ctus = encs[i]->seq.nctu;
	if ((rc = launch_buffers(lead, n, max_ctus, BATCH_MAX))) return rc;
	// frame set-up on the host; nothing is queued on the sequences' streams: the launch's stream waits for what each of them still has in flight (the filter
	// chain and packing of its previous frame) and takes the rest - the frames' parameters in one upload, the phase planes, the per-frame state in one kernel
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		if ((rc = set_frame(e, slots[i], image_types ? image_types[i] : 0, -1.0, false))) return rc;
		e->pic_stream = bst;
		HIP_TRY(hipEventRecord(e->ev_ready, e->ctx->stream));
		if (i) HIP_TRY(hipStreamWaitEvent(bst, e->ev_ready, 0));
		lead->h_frames[i] = e->f;
		lead->h_devs[i] = e->d;
		lead->h_devs[i].frame = lead->d_frames + i;
		rows_total += pool_inflight(e->seq, e->raster);
		needs_rd = needs_rd || e->seq.rd_mode == RDM_FULL;
	}
	// The phase planes of all the reference pictures one after the other on the launch's stream: a picture's three kernels fill the GPU (2500 workgroups, 1.9 TB/s);
	// run side by side on the sequences' streams, sixteen at a time, they reached a quarter of that between them (rocprofv3 trace: 52 ms for 180 pictures).
	// ... luma on the launch's stream, U and V on two side streams: a picture's kernels are 33 + 2 x 20 us of a GPU they do not fill at their ends, three in
	// flight overlap those ends (sixteen thrash, one leaves them exposed)
	if (!lead->plane_stream[0]) {
		for (int k = 0; k < 2; k++) {
			HIP_TRY(hipStreamCreateWithFlags(&lead->plane_stream[k], hipStreamNonBlocking));
			HIP_TRY(hipEventCreateWithFlags(&lead->ev_plane[k], hipEventDisableTiming));
		}
		HIP_TRY(hipEventCreateWithFlags(&lead->ev_plane[2], hipEventDisableTiming));
	}
	HIP_TRY(hipEventRecord(lead->ev_plane[2], bst));
	for (int k = 0; k < 2; k++) HIP_TRY(hipStreamWaitEvent(lead->plane_stream[k], lead->ev_plane[2], 0));
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		const Seq &s = e->seq;
		if (e->f.slice_type == SLICE_I) continue;
		if ((rc = hmr_subpel_plane_on(bst, 0, e->d_pic[e->cur ^ 1][0], s.stride_y, s.height + 2 * s.margin_y, e->planes.y))) return rc;
		for (int k = 0; k < 2; k++)
			if ((rc = hmr_subpel_plane_on(lead->plane_stream[k], 1 + k, e->d_pic[e->cur ^ 1][1 + k], s.stride_c, s.height / 2 + 2 * s.margin_c, e->planes.c[k]))) return rc;
	}
	for (int k = 0; k < 2; k++) {
		HIP_TRY(hipEventRecord(lead->ev_plane[k], lead->plane_stream[k]));
		HIP_TRY(hipStreamWaitEvent(bst, lead->ev_plane[k], 0));
	}
	return submit_staged(lead, n, rows_total, needs_rd);
}

// FINISH: wait for the launch; frame bookkeeping from the gathered counters, distortions and sub-stream sizes; the sub-streams of all pictures packed into one
// staging buffer by one kernel and their download queued on the copy stream
int batch_finish(hmr_gpu_enc **encs, int n, BatchTimes &bt)
{
	hmr_gpu_enc *lead = encs[0];
	hipStream_t bst = lead->ctx->stream;
	int rc;
	float ms = 0;
	if ((rc = wait_for_launch(lead, &ms))) return rc;
	bt.t[2] = std::chrono::steady_clock::now();
	if (!lead->h_offs) HIP_TRY(hipHostMalloc((void **)&lead->h_offs, BATCH_MAX * sizeof(size_t), hipHostMallocDefault));
	lead->pend_off.resize(n);
	lead->pend_rows.assign(n, std::vector<uint32_t>());
	size_t total = 0;
	for (int i = 0; i < n; i++) {
		hmr_gpu_enc *e = encs[i];
		PictureResults res;
		if ((rc = read_record(lead, i, e, "hmr_gpu_enc_encode_batch: sequence", &res))) return rc;
		const int rows = e->seq.wpp ? e->seq.hctu : 1;
		lead->pend_off[i] = total;
		lead->h_offs[i] = total;
		lead->pend_rows[i].assign(res.row_bytes, res.row_bytes + rows);
		for (int r = 0; r < rows; r++) total += lead->pend_rows[i][r];
		total = (total + 255) & ~(size_t)255;
		e->last_ms = e->last_total_ms = ms;
		release_planes(e);
		// the frame's statistics (encoder_engine_thread :3217-3238) need the CTUs' distortions only: the sequence can start its next frame
		e->f_pending = e->f;
		e->awaiting_delivery = true;
		end_frame(e->seq, e->st, e->f, frame_acc_dist(e->seq, e->cfg.wfpp_num_threads, [&](int c) { return res.dist[c]; }), &res.rc);
	}
	if ((rc = grow_pair(&lead->d_stage, &lead->h_stage, &lead->stage_bytes, total, total * 2 + (1 << 20)))) return rc;
	if (!lead->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&lead->copy_stream, hipStreamNonBlocking));
	hipLaunchKernelGGL(k_pack_streams, dim3(n), dim3(256), 0, bst, (const EncDev *)lead->d_batch, lead->d_stage, (const size_t *)lead->h_offs);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(lead->ev_decided, bst));
	HIP_TRY(hipStreamWaitEvent(lead->copy_stream, lead->ev_decided, 0));
	if (total) HIP_TRY(hipMemcpyAsync(lead->h_stage, lead->d_stage, total, hipMemcpyDeviceToHost, lead->copy_stream));
	bt.t[3] = std::chrono::steady_clock::now();
	lead->pend_encs.assign(encs, encs + n);
	lead->pend_total = total;
	lead->pending = true;
	return HMR_GPU_OK;
}

// DELIVER: the outstanding step's access units
int batch_deliver(hmr_gpu_enc *lead, uint8_t **streams, const long *caps, long *stream_bytes, BatchTimes &bt)
{
	const int n = (int)lead->pend_encs.size();
	bt.t[4] = std::chrono::steady_clock::now();
	lead->pending = false;
	for (int i = 0; i < n; i++) lead->pend_encs[i]->awaiting_delivery = false;
	HIP_TRY(hipStreamSynchronize(lead->copy_stream));
	bt.t[5] = std::chrono::steady_clock::now();
	std::vector<int> rcs(n, 0);
	std::vector<std::string> errs(n);
	parallel_for(n, CODING_THREADS, [&](int i) {
		hmr_gpu_enc *e = lead->pend_encs[i];
		rcs[i] = frame_assemble(e, e->f_pending, lead->h_stage + lead->pend_off[i], lead->pend_rows[i].data(), streams[i], caps[i], &stream_bytes[i]);
		if (rcs[i] < 0) errs[i] = hmr_gpu_last_error();
	});
	bt.t[6] = std::chrono::steady_clock::now();
	for (int i = 0; i < n; i++)
		if (rcs[i] < 0) { hmr_set_error("hmr_gpu_enc_encode_batch: sequence %d: %s", i, errs[i].c_str()); return rcs[i]; }
	return HMR_GPU_OK;
}

void batch_report(const BatchTimes &bt, hmr_gpu_enc *lead, bool pipelined)
{
	if (!getenv("HENC_BATCH_TIMING")) return;
	static std::chrono::steady_clock::time_point last_end;
	const auto now = std::chrono::steady_clock::now();
	fprintf(stderr, "batch step%s: launch %.1f ms, wait for the pool %.1f, queue device parts %.1f, download wait %.1f (%.0f MB), entropy coding %.1f; the call %.1f, since the last call %.1f\n",
		pipelined ? " (pipelined)" : "", bt.ms(0, 1), pipelined ? bt.ms(6, 2) : bt.ms(1, 2), bt.ms(2, 3), bt.ms(4, 5), lead->pend_total / 1e6, bt.ms(5, 6),
		std::chrono::duration<double, std::milli>(now - bt.t[0]).count(), std::chrono::duration<double, std::milli>(bt.t[0] - last_end).count());
	last_end = now;
}
}  // namespace

extern "C" int hmr_gpu_enc_encode_batch(hmr_gpu_enc **encs, int n, const int *slots, const int *image_types, uint8_t **streams, const long *caps, long *stream_bytes)
{
	int rc = batch_check(encs, n, slots, streams, caps, stream_bytes);
	if (rc) return rc;
	if (!slots) return HMR_GPU_ERR_ARG;
	for (int i = 0; i < n; i++)
		if (encs[i]->awaiting_delivery || encs[i]->pending) {
			hmr_set_error("hmr_gpu_enc_encode_batch: encoder %d has an access unit outstanding from a pipelined call: flush first", i);
			return HMR_GPU_ERR_ARG;
		}
	hmr_gpu_enc *lead = encs[0];
	HIP_TRY(hipSetDevice(lead->ctx->device));
	BatchTimes bt;
	bt.t[0] = std::chrono::steady_clock::now();
	if ((rc = batch_launch(encs, n, slots, image_types))) return rc;
	bt.t[1] = std::chrono::steady_clock::now();
	if ((rc = batch_finish(encs, n, bt))) return rc;
	if ((rc = batch_deliver(lead, streams, caps, stream_bytes, bt))) return rc;
	batch_report(bt, lead, false);
	return HMR_GPU_OK;
}

// The pipelined form: call k launches the frames slots[] and delivers the access units of call k - 1's frames (stream_bytes[i] = 0 on the first call).
// slots == NULL: deliver the outstanding access units only.  The encoder list stays the same from call to call until the flush.
extern "C" int hmr_gpu_enc_encode_batch_pipelined(hmr_gpu_enc **encs, int n, const int *slots, const int *image_types, uint8_t **streams, const long *caps, long *stream_bytes)
{
	int rc = batch_check(encs, n, slots, streams, caps, stream_bytes);
	if (rc) return rc;
	hmr_gpu_enc *lead = encs[0];
	HIP_TRY(hipSetDevice(lead->ctx->device));
	if (lead->pending) {
		if ((int)lead->pend_encs.size() != n || memcmp(lead->pend_encs.data(), encs, n * sizeof(hmr_gpu_enc *))) {
			hmr_set_error("hmr_gpu_enc_encode_batch_pipelined: the encoder list changed while access units are outstanding: flush (slots = NULL) with the previous list first");
			return HMR_GPU_ERR_ARG;
		}
	} else {
		for (int i = 0; i < n; i++)
			if (encs[i]->awaiting_delivery) {
				hmr_set_error("hmr_gpu_enc_encode_batch_pipelined: encoder %d has an access unit outstanding in another batch", i);
				return HMR_GPU_ERR_ARG;
			}
	}
	BatchTimes bt;
	for (auto &t : bt.t) t = std::chrono::steady_clock::now();
	if (slots && (rc = batch_launch(encs, n, slots, image_types))) return rc;
	bt.t[1] = std::chrono::steady_clock::now();
	if (lead->pending) {
		if ((rc = batch_deliver(lead, streams, caps, stream_bytes, bt))) return rc;
	} else {
		for (int i = 0; i < n; i++) stream_bytes[i] = 0;
		bt.t[6] = bt.t[1];
	}
	if (slots && (rc = batch_finish(encs, n, bt))) return rc;
	if (slots) batch_report(bt, lead, true);
	return HMR_GPU_OK;
}

// Consecutive frames of ONE sequence in one CTU launch, overlapping as far as the reference samples allow (the engines' overlap of the reference, encoder_engine_thread
// hmr_encoder_lib.c:3154-3211 with the row semaphores of :2393-2445, in the interleaving the engine turnstile pins: oracle/ref_ctudump.c:88-108).
// encs[0 .. n - 1]: the engine objects (hmr_gpu_enc_create_engine) of the frames slots[0 .. n - 1] in coding order, n <= num_enc_engines; prev: the object that encoded
// the frame before slots[0] (NULL for the sequence's first frame).  Frame j predicts from the final picture of frame j - 1 where it lies - in encs[j - 1], or prev - and
// from the phase planes the S tasks of that picture's launch have written (enc_post.h); its CTUs of a wavefront step start when the S tasks of the part of the
// reference they can reach are done.  Frame typing and the frame scalars a frame starts from are those of the sequential order: they depend on frames at least n before
// it, except when a frame of the chain detects a scene change - if a later frame of the same chain detects one too, the call fails (HMR_GPU_ERR_ARG) and the chain has
// to be repeated frame by frame.
extern "C" int hmr_gpu_enc_encode_chain(hmr_gpu_enc **encs, int n, hmr_gpu_enc *prev, const int *slots, const int *image_types, uint8_t **streams, const long *caps, long *stream_bytes)
{
	if (!encs || n <= 0 || n > CHAIN_MAX_FRAMES || !slots || !streams || !caps || !stream_bytes) return HMR_GPU_ERR_ARG;
	for (int j = 0; j < n; j++) {
		hmr_gpu_enc *e = encs[j];
		if (!e || !e->lockstep || e->ctx->device != encs[0]->ctx->device || slots[j] < 0 || slots[j] >= (int)e->src.size() || !streams[j] || e->awaiting_delivery || e->engine_index < 0 ||
		    e->seq.width != encs[0]->seq.width || e->seq.height != encs[0]->seq.height) {
			hmr_set_error("hmr_gpu_enc_encode_chain: frame %d: needs an engine object (hmr_gpu_enc_create_engine) of the chain's sequence on the chain's device with a loaded picture slot", j);
			return HMR_GPU_ERR_ARG;
		}
		// rate control and RD_FULL read entropy-coder state of the frame before (rc_end_pic's VBV / QP carry, the context ring of the coder objects): a chain's frames
		// start from a PREDICTED host state, in which neither exists, and the replay check behind the launch would not see a wrong QP - refused, as make_seq refuses
		// them for num_enc_engines > 1 (hmr_rate_control.c:266-282, hmr_encoder_lib.c:3268-3279 are per-frame, in order)
		if (n > 1 && (e->seq.bitrate_mode != 0 || e->seq.rd_mode == RDM_FULL)) {
			hmr_set_error("hmr_gpu_enc_encode_chain: frame %d: rate control and RD_FULL need the frames one at a time (a chain of %d frames starts them from a predicted state)", j, n);
			return HMR_GPU_ERR_ARG;
		}
		// more frames than engines: an engine's next frame is encoded by a twin of its object (hmr_gpu_enc_create_engine_twin: the same persistent engine state)
		if (j >= e->st.engines && e->d_ctus_eng[0] != encs[j - e->st.engines]->d_ctus_eng[0]) {
			hmr_set_error("hmr_gpu_enc_encode_chain: frame %d: the object has to be a twin (hmr_gpu_enc_create_engine_twin) of the one that encodes frame %d, the engine's frame before it", j, j - e->st.engines);
			return HMR_GPU_ERR_ARG;
		}
		for (int i = 0; i < j; i++)
			if (encs[i] == e) return HMR_GPU_ERR_ARG;
	}
	hmr_gpu_enc *lead = encs[0];
	hipStream_t bst = lead->ctx->stream;
	HIP_TRY(hipSetDevice(lead->ctx->device));
	int rc, rows_total = 0;
	bool needs_rd = false;
	if (!lead->d_frames) {
		HIP_TRY(hipMalloc((void **)&lead->d_frames, BATCH_MAX * sizeof(FrameCtx)));
		HIP_TRY(hipHostMalloc((void **)&lead->h_frames, BATCH_MAX * sizeof(FrameCtx), hipHostMallocDefault));
		HIP_TRY(hipHostMalloc((void **)&lead->h_devs, BATCH_MAX * sizeof(EncDev), hipHostMallocDefault));
	}
	if (!lead->d_batch) HIP_TRY(hipMalloc((void **)&lead->d_batch, BATCH_MAX * sizeof(EncDev)));
	// the state every frame starts from, as the sequential order would hand it over: what begin_frame reads of it is older than the chain, a scene change excepted
	HostState st = prev ? prev->st : lead->st;
	const HostState start_state = st;
	// A call that is refused while the frames are being set up leaves every object as it found it: set_frame moves an object on to its next picture buffer and frame
	// state before the checks of the LATER frames of the chain run (wrong engine, a P frame without the object before it, an I frame inside the chain).
	struct Undo { hmr_gpu_enc *e; int cur; HostState st; FrameCtx f; PlaneSet planes, planes2; EncDev d; bool has_picture; hipStream_t pic_stream; };
	std::vector<Undo> undo;
	auto refuse = [&](int code) {
		for (size_t k = undo.size(); k-- > 0;) {
			Undo &u = undo[k];
			u.e->cur = u.cur; u.e->st = u.st; u.e->f = u.f; u.e->chain_planes = u.planes; u.e->chain_planes2 = u.planes2; u.e->d = u.d;
			u.e->has_picture = u.has_picture; u.e->pic_stream = u.pic_stream;
		}
		return code;
	};
	for (int j = 0; j < n; j++) {
		hmr_gpu_enc *e = encs[j];
		const Seq &s = e->seq;
		if (st.num_encoded_frames % e->st.engines != e->engine_index) {
			hmr_set_error("hmr_gpu_enc_encode_chain: frame %d of the sequence belongs to engine %d, not %d", st.num_encoded_frames, st.num_encoded_frames % e->st.engines, e->engine_index);
			return refuse(HMR_GPU_ERR_ARG);
		}
		for (int k = 0; k < 2; k++) {
			PlaneSet &ps = k ? e->chain_planes2 : e->chain_planes;
			if (ps.y) continue;
			PlaneSet p;
			p.device = e->ctx->device; p.bytes_y = (size_t)16 * s.plane_elems_y; p.bytes_c = (size_t)64 * s.plane_elems_c;
			HIP_TRY(hipMalloc((void **)&p.y, p.bytes_y));
			HIP_TRY(hipMalloc((void **)&p.c[0], p.bytes_c));
			HIP_TRY(hipMalloc((void **)&p.c[1], p.bytes_c));
			ps = p;
		}
		undo.push_back(Undo{e, e->cur, e->st, e->f, e->chain_planes, e->chain_planes2, e->d, e->has_picture, e->pic_stream});
		e->st = st;
		// what the frame predicts from, taken before the object that holds it (prev may be the chain's last object) moves on to its own next frame
		const hmr_gpu_enc *r = j ? encs[j - 1] : prev;
		const int16_t *ref_planes[3] = {nullptr, nullptr, nullptr};
		PlaneSet ref_set;
		if (r) {
			for (int c = 0; c < 3; c++) ref_planes[c] = plane0(const_cast<hmr_gpu_enc *>(r), r->cur, c);
			ref_set = r->chain_planes;
		}
		std::swap(e->chain_planes, e->chain_planes2);      // (an object writes its two sets in turn: prev - often the chain's last object - keeps the set the chain's first frame reads)
		if (j == 0 && e == prev) ref_set = e->chain_planes2;       // (a one-engine sequence: the object predicts from its own last picture)
		if ((rc = set_frame(e, slots[j], image_types ? image_types[j] : 0, -1.0, false, true))) return refuse(rc);
		e->pic_stream = bst;
		st = e->st;
		st.num_encoded_frames++;                       // (what end_frame will do; the distortion average it will store is not read inside the chain)
		if (e->f.slice_type != SLICE_I) {
			if (!r || !ref_set.y) {
				hmr_set_error("hmr_gpu_enc_encode_chain: frame %d is a P frame and there is no object that holds the picture before it with its phase planes", j);
				return refuse(HMR_GPU_ERR_ARG);
			}
			for (int c = 0; c < 3; c++) e->f.ref[c] = ref_planes[c];
			e->f.sub_y = ref_set.y + (size_t)s.margin_y * 16 * s.stride_y + s.margin_y;
			e->f.sub_c[0] = ref_set.c[0] + (size_t)s.margin_c * 64 * s.stride_c + s.margin_c;
			e->f.sub_c[1] = ref_set.c[1] + (size_t)s.margin_c * 64 * s.stride_c + s.margin_c;
			e->d.dep = j ? j - 1 : -1;
			e->d.dep_full = getenv("HENC_CHAIN_SERIAL") ? 1 : 0;
		}
		if (j >= e->st.engines) {
			// the engine's second (third ...) frame of the launch: it starts when the one before it is finished, from the average distortion that one leaves
			// (the launch writes it into this frame's parameters); an I frame inside the sequence hands on the value of the frame BEFORE it (end_frame), which
			// the launch does not have
			const hmr_gpu_enc *b = encs[j - e->st.engines];
			if (b->f.slice_type == SLICE_I && b->f.num_encoded_frames != 0 && s.intra_period != 1) {
				hmr_set_error("hmr_gpu_enc_encode_chain: frame %d is an I frame inside the sequence and the same engine's next frame is in the chain: end the chain before frame %d", j - e->st.engines, j);
				return refuse(HMR_GPU_ERR_ARG);
			}
			e->d.after = j - e->st.engines;
			e->f.avg_dist = 0.0;
			lead->h_devs[j - e->st.engines].next_frame = lead->d_frames + j;
		}
		e->d.post.planes[0] = e->chain_planes.y; e->d.post.planes[1] = e->chain_planes.c[0]; e->d.post.planes[2] = e->chain_planes.c[1];
		HIP_TRY(hipEventRecord(e->ev_ready, e->ctx->stream));
		if (j) HIP_TRY(hipStreamWaitEvent(bst, e->ev_ready, 0));
		lead->h_frames[j] = e->f;
		lead->h_devs[j] = e->d;
		lead->h_devs[j].frame = lead->d_frames + j;
		rows_total += s.hctu;
		needs_rd = needs_rd || s.rd_mode == RDM_FULL;
	}
	// (This entry still has its own copy of the launch sequence and reads the records by word index - g[1 .. 11] are GatherHead's members in order, k_encode_object.inc:
	// a rewrite on submit_staged / read_record was taken out again, profiles/launch_collect_refactor.md section 5.  Only the pitch is the shared one: the kernel stores
	// the head's doubles as doubles, which needs gather_pitch's even record size.)
	const int pitch = gather_pitch(lead->seq.nctu);
	if ((size_t)pitch * n > lead->gather_words) {
		if (lead->d_gather) (void)hipFree(lead->d_gather);
		if (lead->h_gather) (void)hipHostFree(lead->h_gather);
		lead->d_gather = lead->h_gather = nullptr;
		lead->gather_words = 0;
		HIP_TRY(hipMalloc((void **)&lead->d_gather, (size_t)pitch * BATCH_MAX * 4));
		HIP_TRY(hipHostMalloc((void **)&lead->h_gather, (size_t)pitch * BATCH_MAX * 4, hipHostMallocDefault));
		lead->gather_words = (size_t)pitch * BATCH_MAX;
	}
	hipLaunchKernelGGL(k_batch_stage, dim3(n), dim3(256), 0, bst, (const EncDev *)lead->h_devs, (const FrameCtx *)lead->h_frames, (EncDev *)lead->d_batch, lead->d_frames);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(lead->ev_batch0, bst));
	if ((rc = launch_pool(lead, lead->h_devs, n, rows_total, needs_rd, bst))) return rc;
	(void)hipEventRecord(lead->ev_batch1, bst);
	hipLaunchKernelGGL(k_gather_results, dim3(n), dim3(256), 0, bst, (const EncDev *)lead->d_batch, lead->d_gather, pitch, (const int *)(lead->d_pool_state + BATCH_MAX * POOL_STRIDE));
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(lead->h_gather, lead->d_gather, (size_t)pitch * n * 4, hipMemcpyDeviceToHost, bst));
	{
		const hipError_t waited = hipStreamSynchronize(bst);
		if (waited != hipSuccess) { hmr_set_error("k_encode_pool: %s", hipGetErrorString(waited)); return HMR_GPU_ERR_HIP; }
	}
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, lead->ev_batch0, lead->ev_batch1));
	// the frames' bookkeeping in coding order, on the state the sequential order hands from frame to frame
	HostState seq_state = start_state;
	bool cut_before = false;
	for (int j = 0; j < n; j++) {
		hmr_gpu_enc *e = encs[j];
		const Seq &s = e->seq;
		const uint32_t *g = lead->h_gather + (size_t)j * pitch;
		if (g[3] & 2) { hmr_set_error("k_encode_pool: the launch was abandoned by its watchdog (HENC_WATCHDOG_S)"); return HMR_GPU_ERR_HIP; }
		if (g[3] & 1) { hmr_set_error("hmr_gpu_enc_encode_chain: frame %d: a CTU row's sub-stream outgrew its buffer (%d bytes)", j, e->row_cap); return HMR_GPU_ERR_HIP; }
		e->note_stale_predictions(g[3] >> 8);
		e->last_ms = e->last_total_ms = ms;
		e->last_encodes = (int)g[1];
		e->f.scene_cut_ctu = (int)g[2];
		e->last_passes = 1;
		const bool fired = (int)g[2] >= 0;
		if (fired && cut_before) {
			hmr_set_error("hmr_gpu_enc_encode_chain: two frames of the chain detected a scene change: in the sequential order the first one switches the detection off for the second; repeat the chain frame by frame");
			return HMR_GPU_ERR_ARG;
		}
		cut_before = cut_before || fired;
		// the frame's true starting state: what begin_frame made of the predicted one (picture order count, frame typing) on top of what the frames before really left
		FrameCtx replay;
		e->st = seq_state;
		begin_frame(s, e->st, image_types ? image_types[j] : 0, replay);
		double acc_dist;
		memcpy(&acc_dist, &g[8], 8);
		memcpy(&e->f.avg_dist, &g[10], 8);      // (what the frame's CTUs read: for an engine's later frames of the launch the launch itself set it)
		if (replay.slice_type != e->f.slice_type || replay.poc != e->f.poc || replay.avg_dist != e->f.avg_dist) {
			hmr_set_error("hmr_gpu_enc_encode_chain: frame %d started from a state the frames before it changed", j);
			return HMR_GPU_ERR_ARG;
		}
		FrameRcOut ro;
		ro.sum_qp = (int)g[4]; ro.consumed_bits = (double)g[5];
		memcpy(&ro.target_pict_size, &g[6], 8);
		end_frame(s, e->st, e->f, acc_dist, &ro);      // (the total the launch formed when the picture finished: by now a twin's frame may have overwritten the records)
		seq_state = e->st;
		// the access unit
		const int rows = s.wpp ? s.hctu : 1;
		std::vector<uint32_t> row_bytes(g + pitch - POST_MAX_ROWS, g + pitch - POST_MAX_ROWS + rows);
		size_t total = 0;
		for (int r = 0; r < rows; r++) total += row_bytes[r];
		if (e->h_bs.size() < total) e->h_bs.resize(total);
		total = 0;
		for (int r = 0; r < rows; r++) {
			HIP_TRY(hipMemcpyAsync(e->h_bs.data() + total, e->d_bs + (size_t)r * e->row_cap, row_bytes[r], hipMemcpyDeviceToHost, bst));
			total += row_bytes[r];
		}
		HIP_TRY(hipStreamSynchronize(bst));
		if ((rc = frame_assemble(e, e->f, e->h_bs.data(), row_bytes.data(), streams[j], caps[j], &stream_bytes[j])) < 0) return rc;
	}
	return HMR_GPU_OK;
}

// HOMER_enc_encode (homer_hevc_enc_api.h:173): host planes in, access unit out
extern "C" int hmr_gpu_enc_encode(hmr_gpu_enc *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, int image_type, uint8_t *stream, long cap, long *stream_bytes,
				  uint8_t *recon)
{
	const int rc = hmr_gpu_enc_load_source(e, 0, y, u, v);
	if (rc) return rc;
	return hmr_gpu_enc_encode_source(e, 0, image_type, stream, cap, stream_bytes, recon);
}
