// rr_host_lens.h -- the thin lens of rr_render_lens as the kernel takes it, and the one function that derives it from a frame's
// constants: the launcher (rr_capi_query.cpp) and the host ray generator (rr_host_lens_rays) both call it, so the rays of
// k_render_lens and the rays the helper hands out come from the same A, B and s.
#pragma once
#include "../../../include/rrdxr.h"

namespace rr {

// A, B: the lens disk's axes in world space, radius * the normalised columns (M0, M4, M8) and (M1, M5, M9) of proj_inv; s: what
// scales GenerateCameraRay's un-normalised vector onto the focal plane, focus_distance / |(M3, M7, M11)|.  pinhole: radius == 0,
// the rays are those of rr_render_samples (A = B = 0, s unused).  A kernel argument of k_render_lens: 32 bytes.
struct LensDev {
    float A[3], B[3];
    float s;
    uint32_t pinhole;
};

// RR_OK, or RR_ERR_INVALID_ARGUMENT for what rr_render_lens refuses of its lens: null pointers, a radius that is not finite
// and >= 0, a focus_distance that is not finite and > 0, a centre column or (radius > 0) an axis column of proj_inv whose length is
// not finite and non-zero, or an s that is not finite and > 0.  fp32, one rounding per operation.
int lens_setup(const rr_scene_constants* c, const rr_lens* lens, LensDev* out);

} // namespace rr
