// Test aid (include/homer_gpu.h section 17): the post-decision stage of one picture from given CTU records.
//
// enc_post.h's tasks (D: units, copy, deblocking; P: SAO statistics, candidates, decision, SAO + CTU syntax through the lane-spread CABAC, offsets, padding; F; the
// scheduler) and subpel_task.h's task S see, in every other test, what the CTU decisions of a whole encode leave for them.  Here the caller chooses that input: the
// records' side-info goes into the encoder's CTU array, their levels into the level buffer, their reconstruction into the reconstruction planes, an 8-bit source into
// a picture slot - and the product's own k_post_frame runs on it, as run_ctu_passes launches it behind k_sched_finish.  Host code only: no __global__ function and no
// instantiation of a task is added, so the product kernels are what they are without this file.
// Host pointers in, uploads, one launch, downloads per call; not a performance path.

namespace {

struct PostTestBufs {
	std::vector<void *> p;
	~PostTestBufs() { for (void *q : p) if (q) (void)hipFree(q); }
	template <class T>
	int alloc(T **out, size_t bytes)
	{
		void *q = nullptr;
		HIP_TRY(hipMalloc(&q, bytes ? bytes : 16));
		p.push_back(q);
		*out = (T *)q;
		return HMR_GPU_OK;
	}
};

constexpr size_t POST_REC_HEAD = 32, POST_REC_SIDE = offsetof(CtuPublic, ctu_number), POST_REC_COEFF = POST_REC_HEAD + POST_REC_SIDE, POST_REC_RECON = POST_REC_COEFF + 6144 * 2;
static_assert(POST_REC_SIDE == 3 * 256 + 2 * 256 + 9 * 256 + 256 + 256 + 2048 + 2048, "a record's side-info is the head of CtuPublic, field by field");
static_assert(POST_REC_RECON + 6144 * 2 + MODE_STATE_BYTES == REC_BYTES, "record layout (oracle/ref_ctudump.c)");
static_assert(sizeof(SaoOffset) == 35 * 4, "include/homer_gpu.h section 17 states [35] int32 per component");

void post_sizes_of(const hmr_gpu_enc *e, hmr_gpu_post_out &o)
{
	const Seq &s = e->seq;
	for (int c = 0; c < 3; c++) o.plane_elems[c] = (int64_t)e->pic_elems[c];
	o.units = (int64_t)e->units_stride * e->units_rows;
	o.phase_bytes[0] = (int64_t)16 * s.plane_elems_y;
	o.phase_bytes[1] = o.phase_bytes[2] = (int64_t)64 * s.plane_elems_c;
	o.nctu = s.nctu; o.rows = s.hctu; o.row_cap = e->row_cap; o.ctx_bytes = CTX_TOTAL + 5;
	o.stride_y = s.stride_y; o.stride_c = s.stride_c; o.margin_y = s.margin_y; o.margin_c = s.margin_c; o.units_stride = e->units_stride; o.reserved = 0;
}

}  // namespace

extern "C" int hmr_gpu_enc_post_sizes(hmr_gpu_enc *e, hmr_gpu_post_out *out)
{
	if (!e || !out) {
		hmr_set_error("hmr_gpu_enc_post_sizes: NULL argument");
		return HMR_GPU_ERR_ARG;
	}
	post_sizes_of(e, *out);
	return HMR_GPU_OK;
}

extern "C" int hmr_gpu_enc_post_records(hmr_gpu_enc *e, int slice_type, int qp, const uint8_t *records, size_t record_bytes, const uint8_t *src_y, const uint8_t *src_u,
					const uint8_t *src_v, int groups, int with_planes, hmr_gpu_post_out *out)
{
	if (!e || !records || !src_y || !src_u || !src_v || !out) {
		hmr_set_error("hmr_gpu_enc_post_records: NULL argument");
		return HMR_GPU_ERR_ARG;
	}
	const Seq &s = e->seq;
	if (groups < 1 || groups > 32) { hmr_set_error("hmr_gpu_enc_post_records: groups %d outside 1 .. 32", groups); return HMR_GPU_ERR_ARG; }
	if (slice_type != SLICE_P && slice_type != SLICE_I) { hmr_set_error("hmr_gpu_enc_post_records: slice_type %d (1 = P, 2 = I)", slice_type); return HMR_GPU_ERR_ARG; }
	if (qp < 0 || qp > 51) { hmr_set_error("hmr_gpu_enc_post_records: qp %d outside 0 .. 51", qp); return HMR_GPU_ERR_ARG; }
	if (record_bytes != (size_t)REC_BYTES * s.nctu) { hmr_set_error("hmr_gpu_enc_post_records: %zu bytes of records, the picture has %d CTUs of %d bytes", record_bytes, s.nctu, REC_BYTES); return HMR_GPU_ERR_ARG; }
	{
		hmr_gpu_post_out want = *out;
		post_sizes_of(e, want);
		if (memcmp(&want, out, offsetof(hmr_gpu_post_out, dbk))) { hmr_set_error("hmr_gpu_enc_post_records: the sizes in `out` are not this encoder's (hmr_gpu_enc_post_sizes)"); return HMR_GPU_ERR_ARG; }
		bool all = out->mvx && out->mvy && out->ref && out->uqp && out->flags && out->sao_recon && out->sao_coded && out->bs && out->bytecnt && out->cumbits && out->ctx && out->saved && out->errors;
		for (int c = 0; c < 3; c++) all = all && out->dbk[c] && out->fin[c] && (!with_planes || out->planes[c]);
		if (!all) { hmr_set_error("hmr_gpu_enc_post_records: a NULL output pointer"); return HMR_GPU_ERR_ARG; }
	}
	hipStream_t st = e->ctx->stream;
	HIP_TRY(hipSetDevice(e->ctx->device));
	int rc = hmr_gpu_enc_load_source(e, 0, src_y, src_u, src_v);
	if (rc) return rc;

	// the frame, as set_frame sets it up for this slice type and QP - on a copy of the sequence state, which stays where it is
	FrameCtx f;
	{
		HostState hs = e->st;
		if (slice_type == SLICE_P && hs.poc == 0) hs.poc = 1;      // (a sequence's first picture is an I picture whatever is asked for)
		begin_frame(s, hs, slice_type == SLICE_I ? IMG_I : IMG_P, f);
	}
	f.qp = qp;
	EncDev dd = e->d;
	for (int c = 0; c < 3; c++) {
		const size_t o = (size_t)(c ? s.margin_c : s.margin_y) * (c ? s.stride_c : s.stride_y) + (c ? s.margin_c : s.margin_y);
		f.src[c] = e->src[0].p[c];
		f.ref[c] = plane0(e, e->cur ^ 1, c);
		f.rec[c] = e->d_rec[c] + o;
		dd.post.fin[c] = plane0(e, e->cur, c);
	}
	dd.post.sao_lambda = e->d_sao_tab + (slice_type == SLICE_I ? 104 : 0);
	dd.post.ctx_after = nullptr;
	dd.post.planes[0] = dd.post.planes[1] = dd.post.planes[2] = nullptr;

	// the records: side-info as the walk leaves it (init_ctu, enc_ctu.h), levels, the reconstruction cropped to the picture
	std::vector<CtuPublic> heads(s.nctu);
	std::vector<int16_t> coeff((size_t)6144 * s.nctu), rec[3];
	for (int c = 0; c < 3; c++) rec[c].assign(e->pic_elems[c], 0);
	for (int n = 0; n < s.nctu; n++) {
		const uint8_t *r = records + (size_t)n * REC_BYTES;
		CtuPublic &h = heads[n];
		memset((void *)&h, 0, sizeof h);
		memcpy((void *)&h, r + POST_REC_HEAD, POST_REC_SIDE);
		const int cx = (n % s.wctu) * 64, cy = (n / s.wctu) * 64;
		const int ctu_w = cx + 64 > s.width ? s.width - cx : 64, ctu_h = cy + 64 > s.height ? s.height - cy : 64;
		h.ctu_number = n; h.x = cx; h.y = cy;
		h.last_valid_partition = (ctu_w != 64 || ctu_h != 64) ? host_raster2abs(((ctu_h >> 2) - 1) * 16 + (ctu_w >> 2) - 1) : NPART - 1;
		h.has_left = cx > 0; h.has_top = cy > 0; h.has_top_left = cx > 0 && cy > 0; h.has_top_right = cy > 0 && n % s.wctu != s.wctu - 1;
		uint32_t intra = 0;
		for (int a = 0; a < NPART; a++) intra += h.pred_mode[a] == PM_INTRA;
		h.intra_parts = slice_type == SLICE_I ? NPART : intra;
		memcpy(coeff.data() + (size_t)n * 6144, r + POST_REC_COEFF, 6144 * 2);
		const int16_t *rr = (const int16_t *)(r + POST_REC_RECON);
		for (int c = 0; c < 3; c++) {
			const int nn = c ? 32 : 64, px = cx >> (c ? 1 : 0), py = cy >> (c ? 1 : 0), pw = c ? s.width / 2 : s.width, ph = c ? s.height / 2 : s.height;
			const int rs = c ? s.stride_c : s.stride_y, m = c ? s.margin_c : s.margin_y;
			int16_t *p = rec[c].data() + (size_t)m * rs + m;
			for (int yy = 0; yy < nn && py + yy < ph; yy++)
				memcpy(p + (size_t)(py + yy) * rs + px, rr + (size_t)yy * nn, (size_t)(px + nn <= pw ? nn : pw - px) * 2);
			rr += nn * nn;
		}
	}
	HIP_TRY(hipMemcpy2DAsync(e->d.ctus, sizeof(CtuInfo), heads.data(), sizeof(CtuPublic), sizeof(CtuPublic), (size_t)s.nctu, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(e->d.coeff, coeff.data(), coeff.size() * 2, hipMemcpyHostToDevice, st));
	for (int c = 0; c < 3; c++) HIP_TRY(hipMemcpyAsync(e->d_rec[c], rec[c].data(), e->pic_elems[c] * 2, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(e->d_frame, &f, sizeof(FrameCtx), hipMemcpyHostToDevice, st));

	// row counters, coder states, error flags from zero (ctu_stage_prepare); poison where the stage's results go
	const size_t nu = (size_t)e->units_stride * e->units_rows;
	HIP_TRY(hipMemsetAsync(e->d_rows, 0, sizeof(PostRow) * s.hctu, st));
	HIP_TRY(hipMemsetAsync(e->d_ent, 0, sizeof(RowEnt) * s.hctu, st));
	HIP_TRY(hipMemsetAsync(e->d_cumbits, 0, sizeof(uint32_t) * s.nctu, st));
	HIP_TRY(hipMemsetAsync(e->d_post_err, 0, sizeof(int) * 4, st));
	for (int c = 0; c < 3; c++) {
		HIP_TRY(hipMemsetAsync(e->d_pre[c], HMR_GPU_POST_POISON, e->pic_elems[c] * 2, st));
		HIP_TRY(hipMemsetAsync(e->d_pic[e->cur][c], HMR_GPU_POST_POISON, e->pic_elems[c] * 2, st));
	}
	HIP_TRY(hipMemsetAsync(e->d_mvx, HMR_GPU_POST_POISON, nu * 2, st));
	HIP_TRY(hipMemsetAsync(e->d_mvy, HMR_GPU_POST_POISON, nu * 2, st));
	HIP_TRY(hipMemsetAsync(e->d_ref, HMR_GPU_POST_POISON, nu, st));
	HIP_TRY(hipMemsetAsync(e->d_qp, HMR_GPU_POST_POISON, nu, st));
	HIP_TRY(hipMemsetAsync(e->d_flags, HMR_GPU_POST_POISON, nu, st));
	HIP_TRY(hipMemsetAsync(e->d_bs, HMR_GPU_POST_POISON, (size_t)e->row_cap * s.hctu, st));
	PostTestBufs bufs;
	if (with_planes)
		for (int c = 0; c < 3; c++) {
			if ((rc = bufs.alloc(&dd.post.planes[c], (size_t)out->phase_bytes[c]))) return rc;
			HIP_TRY(hipMemsetAsync(dd.post.planes[c], HMR_GPU_POST_POISON, (size_t)out->phase_bytes[c], st));
		}

	HIP_TRY(hipFuncSetAttribute((const void *)k_post_frame, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PostScratch)));
	hipLaunchKernelGGL(k_post_frame, dim3(groups), dim3(64), sizeof(PostScratch), st, dd);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(st));

	std::vector<RowEnt> ent(s.hctu);
	HIP_TRY(hipMemcpy(ent.data(), e->d_ent, sizeof(RowEnt) * s.hctu, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy2D(heads.data(), sizeof(CtuPublic), e->d.ctus, sizeof(CtuInfo), sizeof(CtuPublic), (size_t)s.nctu, hipMemcpyDeviceToHost));
	for (int r = 0; r < s.hctu; r++) {
		out->bytecnt[r] = ent[r].bytecnt;
		memcpy(out->ctx + (size_t)r * out->ctx_bytes, ent[r].ctx, out->ctx_bytes);
		memcpy(out->saved + (size_t)r * out->ctx_bytes, ent[r].saved, out->ctx_bytes);
	}
	for (int n = 0; n < s.nctu; n++) {
		memcpy(out->sao_recon + (size_t)n * 3 * 35, heads[n].sao_recon, sizeof heads[n].sao_recon);
		memcpy(out->sao_coded + (size_t)n * 3 * 35, heads[n].sao_coded, sizeof heads[n].sao_coded);
	}
	for (int c = 0; c < 3; c++) {
		HIP_TRY(hipMemcpy(out->dbk[c], e->d_pre[c], e->pic_elems[c] * 2, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(out->fin[c], e->d_pic[e->cur][c], e->pic_elems[c] * 2, hipMemcpyDeviceToHost));
		if (with_planes) HIP_TRY(hipMemcpy(out->planes[c], dd.post.planes[c], (size_t)out->phase_bytes[c], hipMemcpyDeviceToHost));
	}
	HIP_TRY(hipMemcpy(out->mvx, e->d_mvx, nu * 2, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(out->mvy, e->d_mvy, nu * 2, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(out->ref, e->d_ref, nu, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(out->uqp, e->d_qp, nu, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(out->flags, e->d_flags, nu, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(out->bs, e->d_bs, (size_t)e->row_cap * s.hctu, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(out->cumbits, e->d_cumbits, sizeof(uint32_t) * s.nctu, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(out->errors, e->d_post_err, sizeof(int) * 4, hipMemcpyDeviceToHost));
	if (out->errors[2]) { hmr_set_error("hmr_gpu_enc_post_records: k_post_frame gave up after 30 s without a ready task (errors[2])"); return HMR_GPU_ERR_HIP; }
	if (out->errors[0]) { hmr_set_error("hmr_gpu_enc_post_records: a sub-stream ran out of room (errors[0])"); return HMR_GPU_ERR_HIP; }
	return HMR_GPU_OK;
}
