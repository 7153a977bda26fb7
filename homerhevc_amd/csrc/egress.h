// Device egress (k_egress.hip): the frame encoder's final pictures (int16, padded) -> the caller's 8-bit pictures in device memory, and the exact sums of squared
// differences against the int16 source planes of a picture slot; a batch of pictures per launch.
#pragma once
#include "common.h"

#define EGRESS_MAX_JOBS 512          // pictures per launch (the batch calls' limit)
#define EGRESS_MAX_WIDTH 8192        // a workgroup's partial sum stays inside 32 bits up to this width (k_egress.hip)

// one picture of a launch
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

// Algorithmic bytes of one width x height picture through the kernel (tools/egress_bench.py restates it): the final picture is read, the slot's picture is read
// when sums are asked for, the 8-bit picture is written when one is asked for.
static inline double hmr_egress_bytes(int width, int height, int picture, int sums)
{
	const double wh = (double)width * height;
	return 3.0 * wh + (sums ? 3.0 * wh : 0.0) + (picture ? 1.5 * wh : 0.0);
}

// The job table goes from page-locked host memory (`h_jobs`, which must stay untouched until the work queued here has run) to `d_jobs`, then ONE launch of k_egress handles
// all n pictures; both on `stream`, nothing is waited for.
int hmr_egress_launch(hipStream_t stream, const EgressJob *h_jobs, EgressJob *d_jobs, int n);
