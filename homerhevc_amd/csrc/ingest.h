// Device ingest (k_ingest.hip): 8-bit pictures in device memory -> the int16 source planes of the frame encoder, a batch of pictures per launch.
#pragma once
#include "common.h"

#define INGEST_MAX_JOBS 512          // pictures per launch (the batch calls' limit)

// one picture of a launch
struct IngestJob {
	const uint8_t *src[3];       // I420: Y, U, V; NV12: Y, interleaved UV, unused
	int64_t pitch[3];            // bytes from row to row
	int16_t *dst[3];             // the slot's planes
	int32_t stride_y, stride_c;  // elements, multiples of 8
	int32_t width, height, format, reserved;
};

// The job table goes from page-locked host memory (`h_jobs`, which must stay untouched until the work queued here has run) to `d_jobs`, then ONE launch of k_ingest converts
// all n pictures; both on `stream`, nothing is waited for.
int hmr_ingest_launch(hipStream_t stream, const IngestJob *h_jobs, IngestJob *d_jobs, int n);
